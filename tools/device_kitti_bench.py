"""Detections -> KITTI annotations: the file chain against the device path, in one process.

64 frames (8 ``decode_device``-shaped buffers of 8 samples, N = 3000 rows each) with 50 and with 498 detections per
frame, random boxes 12-90 m ahead of the camera, all ten classes, scores uniform in [0.2, 0.9); the calibration file of
tests/golden/result2kitti.npz.  Reported per case:

  file_chain_ms_per_frame    host time of ``RoadSideEvaluator.format_results`` + ``result2kitti`` + ``get_label_annos``
                             (the detections already in host memory), and its three parts
  device_ms_per_frame        host time of 8 x ``KittiDetections.add_packed`` + ``annos()`` (wall clock, the wait included)
  kernel_us                  the kernel alone on one buffer of 8 samples: HIP events, median of 10 after warm-up

The file chain in this same run is the baseline; no target is fixed in advance.  Prints one JSON line and writes it to
profiles/device_kitti_bench.json (``--out``).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgv3d_amd import _lib, synthetic as S  # noqa: E402
from sgv3d_amd.evaluators import RoadSideEvaluator, result2kitti  # noqa: E402
from sgv3d_amd.evaluators.device_kitti import KittiDetections  # noqa: E402
from sgv3d_amd.evaluators.kitti_utils import kitti_common as KC  # noqa: E402

FRAMES, BATCH, N = 64, 8, 3000


def detections(count, seed):
    g = np.random.default_rng(seed)
    boxes = np.zeros((BATCH, N, 9), np.float32)
    for k, (lo, hi) in enumerate(((12, 90), (-15, 15), (-2, 0), (0.5, 6), (0.4, 2.5), (0.5, 3), (-3.5, 3.5))):
        boxes[..., k] = g.uniform(lo, hi, (BATCH, N))
    scores = g.uniform(0.2, 0.9, (BATCH, N)).astype(np.float32)
    labels = g.integers(0, 10, (BATCH, N)).astype(np.int32)
    return boxes, scores, labels, np.full(BATCH, count, np.int32)


def pack(boxes, scores, labels, counts, dev):
    raw = np.concatenate([a.reshape(-1).view(np.uint8) for a in (boxes, scores, labels, counts)])
    return torch.from_numpy(raw).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_kitti_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device('cuda:0')
    lib = _lib.load()
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'result2kitti.npz'))
    res = dict(frames=FRAMES, batch=BATCH, rows_per_sample=N, score_threshold=0.45)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'dair-v2x-i-kitti')
        os.makedirs(os.path.join(root, 'training', 'calib'))
        for i in range(FRAMES):
            with open(os.path.join(root, 'training', 'calib', f'{i:06d}.txt'), 'w') as f:
                f.write(str(gold['calib_text'][0]))
        metas = [dict(token=f'training/image_2/{i:06d}.jpg', ego2global_translation=[0, 0, 0], ego2global_rotation=[1, 0, 0, 0])
                 for i in range(FRAMES)]
        ev = RoadSideEvaluator(class_names=S.CLASSES, current_classes=['Car', 'Pedestrian', 'Cyclist'], data_root=root,
                               gt_label_path=os.path.join(tmp, 'gt'))
        for count in (50, 498):
            batches = [detections(count, 1000 * count + k) for k in range(FRAMES // BATCH)]
            host = [(b[i, :count], s[i, :count], l[i, :count]) for b, s, l, _ in batches for i in range(BATCH)]
            # ---- file chain -------------------------------------------------------------------------------------------
            t0 = time.perf_counter()
            files, _ = ev.format_results(host, metas, jsonfile_prefix=os.path.join(tmp, f'json{count}'))
            t1 = time.perf_counter()
            folder = result2kitti(files['img_bbox'], os.path.join(tmp, f'out{count}'), root, 'unused')
            t2 = time.perf_counter()
            want, ids = KC.get_label_annos(folder, return_ids=True)
            t3 = time.perf_counter()
            # ---- device path ------------------------------------------------------------------------------------------
            packed = [pack(*b, dev) for b in batches]
            max_det = 512
            warm = KittiDetections(S.CLASSES, data_root=root, max_det=max_det)        # code object, pinned pool, allocator
            warm.add_packed(packed[0], metas[:BATCH])
            warm.annos()
            walls = []
            for _ in range(5):
                dets = KittiDetections(S.CLASSES, data_root=root, max_det=max_det)
                dets._calib, dets._free = warm._calib, warm._free                     # a second epoch: files read, buffers pinned
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                for k, p in enumerate(packed):
                    dets.add_packed(p, metas[k * BATCH:(k + 1) * BATCH])
                got, got_ids = dets.annos()
                walls.append(time.perf_counter() - t4)
                warm._free = dets._free
            same = got_ids == ids and all(g[k].tobytes() == w[k].tobytes() for g, w in zip(got, want) for k in w)
            kept = sum(len(a['name']) for a in got)
            # ---- the kernel alone ---------------------------------------------------------------------------------------
            p = packed[0].data_ptr()
            calib = torch.from_numpy(dets._blocks(metas[:BATCH], None)).to(dev)
            out = torch.empty(BATCH * 4 + BATCH * max_det * 4 + BATCH * max_det * 13 * 8, dtype=torch.uint8, device=dev)
            nws = lib.sgv3d_detections_to_kitti_workspace_bytes(BATCH, N)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            o = out.data_ptr()

            def launch():
                rc = lib.sgv3d_detections_to_kitti(BATCH, N, p, p + BATCH * N * 36, 0, p + BATCH * N * 40, p + BATCH * N * 44,
                                                   calib.data_ptr(), dets.table.ctypes.data, len(dets.table), 0.45, 1920, 1080, max_det, 4,
                                                   ws.data_ptr(), nws, o, o + BATCH * max_det * 104, o + BATCH * max_det * 108,
                                                   _lib.stream_handle(dev))
                _lib.check(rc, "sgv3d_detections_to_kitti")
            for _ in range(5):
                launch()
            us = []
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                us.append(a.elapsed_time(b) * 1e3)
            chain = (t3 - t0) * 1e3 / FRAMES
            device = statistics.median(walls) * 1e3 / FRAMES
            res[f'det{count}'] = dict(
                detections_per_frame=count, kept_per_frame=round(kept / FRAMES, 1), annos_identical=bool(same),
                file_chain_ms_per_frame=round(chain, 3), format_results_ms_per_frame=round((t1 - t0) * 1e3 / FRAMES, 3),
                result2kitti_ms_per_frame=round((t2 - t1) * 1e3 / FRAMES, 3), get_label_annos_ms_per_frame=round((t3 - t2) * 1e3 / FRAMES, 3),
                device_ms_per_frame=round(device, 4), device_ms_per_frame_min_max=[round(min(walls) * 1e3 / FRAMES, 4),
                                                                                    round(max(walls) * 1e3 / FRAMES, 4)],
                kernel_us_batch8=round(statistics.median(us), 1), kernel_us_min_max=[round(min(us), 1), round(max(us), 1)],
                file_chain_over_device=round(chain / device, 1))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
