"""The renderer (csrc/render.hip) on 1080 x 1920 frames: batch 1 and 8, 20 and 200 kept boxes per frame placed on the ground in
front of ``synthetic.make_calib``'s roadside cameras, with ``pcd_vis``'s 1001 x 1201 BEV canvas.  HIP events around
``draw_packed`` (the upload and the three launches), median of 10 after warm-up; in the same run ``frames.clone()`` and
``JpegEncoder`` on the same frames, and the C entry alone.  The kernels are checked against ``sgv3d_render_detections_host`` on
the first frame.  The one-thread CPU figure is tests/render_ref.py on one frame.  Prints one JSON line (kept as
profiles/render_bench.json).

    python tools/render_bench.py [--out profiles/render_bench.json]   # the measurement
    python tools/render_bench.py --profile       # only batch-8 calls at 200 boxes, for `rocprofv3 --kernel-trace --stats`
    python tools/render_bench.py --kernel-stats profiles/render_kernel_stats.csv --out profiles/render_bench.json
                                                 # no GPU: adds the three kernels' times of that trace to the JSON, and the
                                                 # paint launch's share of the HBM peak (its bytes over its own time)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

from sgv3d_amd import render, synthetic as S  # noqa: E402
from sgv3d_amd.jpeg_encode import JpegEncoder  # noqa: E402

HW = (1080, 1920)
HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


def median_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def make_frames(batch, seed=7):
    """Smooth synthetic scenes: a gradient sky, a textured ground."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:HW[0], 0:HW[1]]
    out = np.empty((batch, HW[0], HW[1], 3), np.uint8)
    for b in range(batch):
        base = np.stack([90 + 60 * np.sin(x / (97.0 + b)) * np.cos(y / 131.0), 110 + 0.08 * y, 140 - 0.05 * x + 20 * np.sin(y / 53.0)], -1)
        out[b] = np.clip(base + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8)
    return out


def make_packed(batch, kept, n_rows, seed=3):
    """A buffer in decode_device's layout: ``kept`` rows per frame above the threshold and of mapped classes, the rest below."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((batch, n_rows, 9), np.float32)
    boxes[..., 0] = rng.uniform(12, 95, (batch, n_rows))
    boxes[..., 1] = rng.uniform(-25, 25, (batch, n_rows))
    boxes[..., 2] = rng.uniform(-0.2, 0.2, (batch, n_rows))
    boxes[..., 3] = rng.uniform(3.5, 5.0, (batch, n_rows))
    boxes[..., 4] = rng.uniform(1.6, 2.1, (batch, n_rows))
    boxes[..., 5] = rng.uniform(1.4, 1.9, (batch, n_rows))
    boxes[..., 6] = rng.uniform(-3.1, 3.1, (batch, n_rows))
    scores = np.full((batch, n_rows), 0.2, np.float32)
    labels = rng.integers(0, len(S.CLASSES), (batch, n_rows)).astype(np.int32)
    for b in range(batch):
        rows = rng.permutation(n_rows)[:kept]
        scores[b, rows] = rng.uniform(0.5, 0.99, kept)
        labels[b, rows] = rng.choice([0, 1, 3, 8, 7], kept)               # car, truck, bus, pedestrian, bicycle
    counts = np.full(batch, n_rows, np.int32)
    return np.concatenate([a.reshape(-1).view(np.uint8) for a in (boxes, scores, labels, counts)]), (boxes, scores, labels, counts)


def calibs(batch):
    out = []
    for b in range(batch):
        c = S.make_calib(pitch_deg=11.0 + 0.5 * b, cam_h=5.5 + 0.2 * b, yaw_deg=0.5 * b)
        out.append((np.linalg.inv(c['sensor2ego'].astype(np.float64))[:3], c['intrin'][:3, :3].astype(np.float64)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--kernel-stats', default=None, help="rocprofv3's kernel_stats.csv of a --profile run, merged into --out")
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as f:
            res = json.loads(f.read())
        us = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for name in ('render_setup_kernel', 'render_bin_kernel', 'render_paint_kernel'):
                    if name in row['Name']:
                        us[name] = float(row['AverageNs']) / 1e3
        assert len(us) == 3, us
        res['kernel_trace'] = dict(source='rocprofv3 --kernel-trace --stats of --profile (batch 8, 200 kept boxes, out of place), a run of its own',
                                   **{k + '_us': round(v, 1) for k, v in us.items()})
        moved = res['b8_bytes_moved_out_of_place']
        res['kernel_trace']['paint_launch_share_of_hbm_peak'] = round(moved / (us['render_paint_kernel'] * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
        line = json.dumps(res)
        print(line)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
        return
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    host_frames = make_frames(8)
    frames = torch.from_numpy(host_frames).to(dev)
    canvas = render.BevCanvas()
    r = render.DetectionRenderer(S.CLASSES, src_hw=HW, max_boxes=256, bev=canvas)
    metas = [dict(token=f'{i:06d}') for i in range(8)]
    cal = calibs(8)
    if args.profile:
        raw, _ = make_packed(8, 200, 300)
        packed = torch.from_numpy(raw).to(dev)
        for _ in range(5):
            r.draw_packed(frames, packed, metas, calib=cal)
        torch.cuda.synchronize()
        print("profile run done")
        return
    import render_ref as R
    res = dict(frame_hw=list(HW), bev_hw=[canvas.height, canvas.width], rows_per_frame=300, max_boxes=256, thickness=2,
               method='HIP events, median of 10 after 3 warm-up calls; all figures from one run',
               hbm_peak_gbs=HBM_PEAK_GBS)
    enc = JpegEncoder(HW, quality=95, max_bytes=1 << 22, device=dev)
    for b in (1, 8):
        fb = frames[:b]
        res[f'b{b}_clone_ms_per_frame'] = round(median_ms(lambda: fb.clone()) / b, 4)
        assert enc(fb).status().tolist() == [0] * b
        res[f'b{b}_jpeg_encoder_ms_per_frame'] = round(median_ms(lambda: (enc(fb), torch.cuda.synchronize())) / b, 3)
        for kept in (20, 200):
            raw, (boxes, scores, labels, counts) = make_packed(b, kept, 300)
            packed = torch.from_numpy(raw).to(dev)
            out = r.draw_packed(fb, packed, metas[:b], calib=cal[:b])
            assert out.status().tolist() == [0] * b
            if b == 1:
                cfg = dict(R.config(2, False, max_boxes=256), table=render.class_table(S.CLASSES, render.category_map_dair),
                           class_colors=render.default_class_colors(S.CLASSES).tolist(),
                           bev=dict(w=canvas.width, h=canvas.height, res=canvas.res, x_off=canvas.x_off, y_off=canvas.y_off))
                blocks = np.stack([render.calib_block(*c) for c in cal[:1]])
                want = R.host_twin(cfg, boxes, scores, labels, counts, blocks, host_frames[:1])
                assert np.array_equal(out.frames.cpu().numpy(), want[0]) and np.array_equal(out.bev.cpu().numpy(), want[1]), \
                    "the kernels differ from the host entry"
                res[f'k{kept}_pixels_drawn_frame0'] = int((want[0] != host_frames[:1]).any(-1).sum())
                if kept == 20:
                    t = time.perf_counter()
                    ref = R.render(cfg, boxes, scores, labels, counts, blocks, host_frames[:1])
                    res['k20_numpy_restatement_one_thread_ms_per_frame'] = round((time.perf_counter() - t) * 1e3, 1)
                    assert np.array_equal(ref[0], want[0])
            dst = torch.empty_like(fb)
            ms = median_ms(lambda: r.draw_packed(fb, packed, metas[:b], calib=cal[:b], out=dst))
            res[f'b{b}_k{kept}_draw_packed_ms_per_frame'] = round(ms / b, 4)
            mine = fb.clone()
            ms = median_ms(lambda: r.draw_packed(mine, packed, metas[:b], calib=cal[:b], out=mine))
            res[f'b{b}_k{kept}_draw_packed_in_place_ms_per_frame'] = round(ms / b, 4)
        # the bytes an out-of-place call has to move: the frame read and written, the canvas written.  The share below is of
        # the WHOLE call (staging, upload, three launches); the paint launch alone comes from the kernel trace (--kernel-stats)
        moved = b * (2 * HW[0] * HW[1] * 3 + canvas.height * canvas.width * 3)
        res[f'b{b}_bytes_moved_out_of_place'] = moved
        res[f'b{b}_k200_whole_call_share_of_hbm_peak'] = round(moved / (res[f'b{b}_k200_draw_packed_ms_per_frame'] * b * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
        res[f'b{b}_clone_share_of_hbm_peak'] = round(b * 2 * HW[0] * HW[1] * 3 / (res[f'b{b}_clone_ms_per_frame'] * b * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
    res['render_not_slower_than_jpeg_encoder_at_b8'] = bool(res['b8_k200_draw_packed_ms_per_frame'] <= res['b8_jpeg_encoder_ms_per_frame'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    assert res['render_not_slower_than_jpeg_encoder_at_b8'], "the render call costs more than JpegEncoder on the same frames"


if __name__ == '__main__':
    main()
