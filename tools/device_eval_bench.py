"""KITTI AP tables: the host path (``kitti_eval``) against the device path (``kitti_eval_device``), in one process.

Two synthetic validation sets of 2000 frames: 20 ground-truth boxes and 30 detections per frame, and 50 and 60.  Cars,
pedestrians and cyclists with vans, sitting persons and DontCare regions; the detections are the ground truth jittered,
some dropped, padded with false positives.  Both paths run on the same annotation lists, alternating, five times after a
warm-up of each; medians are reported:

  host_s                  wall time of ``kitti_eval``, and inside it ``clean_data``, ``calculate_overlaps`` (the rotated-box
                          kernel with its copies, and the numpy 2-D overlaps) and the ``sgv3d_kitti_eval_curves`` calls
  device_s                wall time of ``kitti_eval_device`` on the two lists, packing both sides included: what
                          ``evaluate_detections(..., device_eval=True)`` costs, and the ratio reported as host_over_device
  device_prepacked_s      the same with the ground truth packed once ahead (``pack_ground_truth``), as an epoch loop can;
                          the one-time packing is gt_pack_s
  device_events_ms        HIP events around ``curves_device``: upload, launches and download of an already packed input

The two texts must be equal.  The host path of this same run is the baseline; no ratio is fixed in advance.  Prints one
JSON line and writes it to profiles/device_eval_bench.json (``--out``).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgv3d_amd import _lib  # noqa: E402
from sgv3d_amd.evaluators import device_eval as DE  # noqa: E402
from sgv3d_amd.evaluators.kitti_utils import eval as E  # noqa: E402

CLASSES = ['Car', 'Pedestrian', 'Cyclist']


def synthetic(frames, n_gt, n_dt, seed):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(frames):
        n = n_gt
        x1, y1 = rng.uniform(0, 1700, n), rng.uniform(100, 800, n)
        w, h = rng.uniform(40, 200, n), rng.uniform(20, 150, n)
        g = {'name': rng.choice(['Car', 'Car', 'Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare'], n).astype('<U14'),
             'truncated': rng.choice([0.0, 0.0, 0.2, 0.4], n), 'occluded': rng.choice([0.0, 0.0, 1.0, 2.0], n),
             'alpha': rng.uniform(-3, 3, n), 'bbox': np.stack([x1, y1, x1 + w, y1 + h], 1),
             'dimensions': np.stack([rng.uniform(1, 4.5, n), rng.uniform(1.4, 1.9, n), rng.uniform(0.6, 1.9, n)], 1),
             'location': np.stack([rng.uniform(-40, 40, n), rng.uniform(0.8, 1.4, n), rng.uniform(10, 120, n)], 1),
             'rotation_y': rng.uniform(-3, 3, n), 'score': np.zeros(n)}
        keep = np.flatnonzero(rng.uniform(size=n) < 0.85)[:n_dt]
        extra = n_dt - len(keep)
        src = np.concatenate([keep, rng.integers(0, n, extra)])
        d = {k: v[src].copy() for k, v in g.items()}
        d['name'] = np.array(['Car' if x in ('Van', 'DontCare', 'Person_sitting') else x for x in d['name']], dtype='<U14')
        jitter = np.concatenate([np.ones(len(keep)), np.full(extra, 12.0)])          # the padding lands elsewhere: false positives
        d['bbox'] += rng.normal(0, 3, (n_dt, 4)) * jitter[:, None]
        d['location'] += rng.normal(0, 0.15, (n_dt, 3)) * jitter[:, None]
        d['rotation_y'] += rng.normal(0, 0.05, n_dt)
        d['alpha'] += rng.normal(0, 0.1, n_dt)
        d['score'] = np.round(rng.uniform(0.05, 1, n_dt), 3)
        d['truncated'], d['occluded'] = np.zeros(n_dt), np.zeros(n_dt)
        gts.append(g)
        dts.append(d)
    return gts, dts


class Split:
    """Wall time spent inside three parts of the host path, by wrapping them for one call."""

    def __init__(self):
        self.t = dict(clean_data=0.0, overlaps=0.0, curves=0.0)

    def _wrap(self, key, fn):
        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t[key] += time.perf_counter() - t0
        return timed

    def __enter__(self):
        lib = _lib.load()
        self.saved = (E.clean_data, E.calculate_overlaps, lib.sgv3d_kitti_eval_curves)
        E.clean_data = self._wrap('clean_data', self.saved[0])
        E.calculate_overlaps = self._wrap('overlaps', self.saved[1])
        lib.sgv3d_kitti_eval_curves = self._wrap('curves', self.saved[2])
        return self

    def __exit__(self, *exc):
        E.clean_data, E.calculate_overlaps, _lib.load().sgv3d_kitti_eval_curves = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_eval_bench.json'))
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device-only', action='store_true', help='skip the host path (kernel traces)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    res = dict(frames=args.frames, repeats=args.repeats, classes=CLASSES)
    for n_gt, n_dt in ((20, 30), (50, 60)):
        gts, dts = synthetic(args.frames, n_gt, n_dt, seed=n_gt)
        t0 = time.perf_counter()
        packed_gt = DE.pack_ground_truth(gts)
        gt_pack = time.perf_counter() - t0
        device_text, _ = DE.kitti_eval_device(gts, dts, CLASSES)                       # warm-up of each path
        host_text = None if args.device_only else E.kitti_eval(gts, dts, CLASSES)[0]
        assert args.device_only or host_text == device_text, "the two reports differ"
        _, classes, min_overlaps, _ = E.eval_setup(gts, dts, CLASSES, ['bbox', 'bev', '3d'])
        packed = DE.pack_annotations(packed_gt, dts, pinned=True)
        host, device, prepacked, events, parts = [], [], [], [], []
        for _ in range(args.repeats):
            if not args.device_only:
                with Split() as split:
                    t0 = time.perf_counter()
                    text = E.kitti_eval(gts, dts, CLASSES)[0]
                    host.append(time.perf_counter() - t0)
                parts.append(split.t)
                assert text == device_text
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            text = DE.kitti_eval_device(gts, dts, CLASSES)[0]
            device.append(time.perf_counter() - t0)
            assert text == device_text
            t0 = time.perf_counter()
            text = DE.kitti_eval_device(packed_gt, dts, CLASSES)[0]
            prepacked.append(time.perf_counter() - t0)
            assert text == device_text
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            DE.curves_device(packed, classes, min_overlaps, True)
            b.record()
            b.synchronize()
            events.append(a.elapsed_time(b))
        med = statistics.median
        case = dict(gt_per_frame=n_gt, dt_per_frame=n_dt, texts_identical=not args.device_only, gt_pack_s=round(gt_pack, 3),
                    device_s=round(med(device), 4), device_s_min_max=[round(min(device), 4), round(max(device), 4)],
                    device_prepacked_s=round(med(prepacked), 4),
                    device_prepacked_s_min_max=[round(min(prepacked), 4), round(max(prepacked), 4)],
                    device_events_ms=round(med(events), 3), device_events_ms_min_max=[round(min(events), 3), round(max(events), 3)],
                    car_3d_moderate_line=[ln for ln in device_text.splitlines() if ln.startswith('3d')][0])
        if not args.device_only:
            case.update(host_s=round(med(host), 3), host_s_min_max=[round(min(host), 3), round(max(host), 3)],
                        host_clean_data_s=round(med([p['clean_data'] for p in parts]), 3),
                        host_overlaps_s=round(med([p['overlaps'] for p in parts]), 3),
                        host_curves_s=round(med([p['curves'] for p in parts]), 3),
                        host_over_device=round(med(host) / med(device), 1),
                        host_over_device_prepacked=round(med(host) / med(prepacked), 1))
        res[f'gt{n_gt}_dt{n_dt}'] = case
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
