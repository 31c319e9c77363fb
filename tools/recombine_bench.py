"""Time the frame recombination (csrc/recombine.hip) at the shipped DAIR size: generated frames of 1080 x 1920 from three
sources each, batch 8, and print one JSON line.

GPU: HIP events around one ``FrameRecombiner.combine`` call on frames that are already on the device (the descriptors'
upload, the four launches and the copy of the labels to pinned memory), median of ``--iters`` calls after ``--warmup``;
per generated frame the microseconds and the rate on the unique bytes (S source frames and masks read, one frame and
mask read and written).  Baseline: tests/recombine_ref.py, the numpy float64 restatement of the reference's
recombine_utils.py, on one CPU thread for one generated frame of the same run; its frame, mask and label text are
compared with the device's.

    python tools/recombine_bench.py [--batch 8] [--iters 10] [--out profiles/recombine_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recombine_ref as R            # noqa: E402
import recombine_util as U           # noqa: E402
from sgv3d_amd import recombine as RC  # noqa: E402

HW = (1080, 1920)
S = 3


def unique_bytes(h, w, s):
    px = h * w
    return s * (px * 3 + px) + 2 * (px * 3 + px)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--objects', type=int, default=12, help='objects per frame')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), "recombine_bench needs the GPU"
    torch.set_num_threads(1)
    dev = torch.device('cuda', 0)
    h, w = HW
    jobs = [U.make_scene(100 + b, h, w, n_src=S, n_dest_obj=a.objects // 2, n_src_obj=a.objects) for b in range(a.batch)]
    on_dev = {id(f): dict(f, image=torch.from_numpy(f['image']).to(dev), mask=torch.from_numpy(f['mask']).to(dev))
              for d, srcs in jobs for f in [d] + srcs}
    frames = [on_dev[id(f)] for d, srcs in jobs for f in [d] + srcs]
    pool = (torch.stack([f['image'] for f in frames]), torch.stack([f['mask'] for f in frames]))
    for i, f in enumerate(frames):
        f['index'] = i
    dest = [on_dev[id(d)] for d, _ in jobs]
    sources = [[on_dev[id(s)] for s in srcs] for _, srcs in jobs]
    rec = RC.FrameRecombiner(src_hw=HW, max_sources=S, max_obj=64)
    for _ in range(a.warmup):
        res = rec.combine(dest, sources, pool=pool)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = rec.combine(dest, sources, pool=pool)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)
    us_call = float(np.median(times))
    labels = res.labels()
    nbytes = unique_bytes(h, w, S)
    out = {'metric': f'frame recombination {h}x{w}, {S} sources per generated frame, batch {a.batch} (warp + brightness + gate + paste + labels)',
           'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'sources': S, 'iters': a.iters,
           'us_per_call_median': round(us_call, 1), 'us_per_call_min': round(min(times), 1), 'us_per_call_max': round(max(times), 1),
           'us_per_frame': round(us_call / a.batch, 1), 'unique_bytes_per_frame': nbytes,
           'TBps_on_unique_bytes': round(nbytes * a.batch / (us_call * 1e-6) / 1e12, 3),
           'accepted_objects_per_frame': [int(l['kept'].sum()) for l in labels],
           'pasted_pixels_frame0': int((res.frames[0] != pool[0][dest[0]['index']]).any(-1).sum())}
    if not a.no_cpu:
        t = time.perf_counter()
        ref = R.recombine(*jobs[0])
        cpu_s = time.perf_counter() - t
        near = np.zeros(ref['image'].shape, bool)
        for v in ref['shifted_abs']:
            near |= np.abs(v - (np.floor(v) + 0.5)) <= 1e-6
        out['cpu_numpy_one_frame_ms'] = round(cpu_s * 1e3, 1)
        out['cpu_threads'] = 1
        out['speedup_per_frame'] = round(cpu_s * 1e6 / (us_call / a.batch), 1)
        out['matches_cpu'] = {'labels': labels[0]['lines'] == ref['lines'], 'mask': bool(np.array_equal(res.masks[0].cpu().numpy(), ref['mask'])),
                              'image_away_from_ties': bool(np.array_equal(res.frames[0].cpu().numpy()[~near], ref['image'][~near])),
                              'values_near_a_tie': int(near.sum())}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
