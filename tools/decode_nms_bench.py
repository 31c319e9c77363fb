"""The on-device box decode (BEVHeightHead.decode_device: candidate stage, NMS, task merge -- four launches) with
``nms_type='circle'`` and ``nms_type='rotate'`` on cfg-2-sized head maps (six tasks, 256 x 256, max_num 500, 40 Gaussian
blobs per task and sample over low background heat, as tests/test_decode_gpu.py builds them), batch 1 and batch 8.

µs per call from HIP events after warm-up: the two types alternate in the same process, ``--rounds`` rounds of ``--iters``
calls each, median and spread over the rounds.  The circle path is the parent's, kernel for kernel; the ratio
rotate / circle is the cost of switching.  Four more rotate decodes take the NMS launch apart from outside:
``rotate_pre1`` (pre_max_size = 1: the candidate stage, the compaction and the merge, no pair and no walk),
``rotate_post1`` (post_max_size = 1: everything but the walk, which ends at the second live candidate), ``rotate_noclip``
(the same maps with every extent shrunk to nothing and no post_max_size: the circle test of every pair, no clipping, and
the longest walk there is, n kept candidates) and ``rotate_noclip_post1`` (circle test alone).  So rotate - rotate_post1
is the walk, rotate_post1 - rotate_noclip_post1 the clipping, rotate_noclip_post1 - rotate_pre1 the circle test.
Per-kernel times come from a separate run under the profiler (tracing slows
the host, so the two are never taken together):

    python tools/decode_nms_bench.py --profile --batch 8            # under `rocprofv3 --kernel-trace --stats ... --`
    python tools/decode_nms_bench.py --kernel-stats 8=<kernel_stats.csv> --kernel-stats 1=<...> --out profiles/decode_rotate_bench.json

Prints one JSON line (kept as profiles/decode_rotate_bench.json).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgv3d_amd import synthetic as S  # noqa: E402
from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead  # noqa: E402

H = W = 256
KERNELS = ('topk_per_class_kernel', 'merge_decode_kernel', 'circle_nms_kernel', 'rotate_nms_kernel', 'merge_tasks_kernel')


KINDS = ('circle', 'rotate', 'rotate_pre1', 'rotate_post1', 'rotate_noclip', 'rotate_noclip_post1')


def heads():
    out = {}
    for kind in KINDS:
        _, hc = S.r50_256_conf()
        hc['test_cfg'] = dict(hc['test_cfg'], nms_type=kind.split('_')[0])
        if kind == 'rotate_pre1':
            hc['test_cfg']['pre_max_size'] = 1
        if kind == 'rotate_noclip':
            hc['test_cfg']['post_max_size'] = None
        if kind.endswith('_post1'):
            hc['test_cfg']['post_max_size'] = 1
        out[kind] = BEVHeightHead(**hc)
    return out


def fake_preds(B, H, W, seed, n_obj=40):
    """Head-like maps in one buffer: low background heat with n_obj Gaussian blobs per task and sample.  Returns the buffer
    and, per task, {map name: (channel offset, channels)}."""
    g = np.random.default_rng(seed)
    names = [('reg', 2), ('height', 1), ('dim', 3), ('rot', 2), ('vel', 2)]
    ncls = [1, 2, 2, 1, 2, 2]
    buf = g.standard_normal((B, 70, H, W)).astype(np.float32) * 0.3
    preds, off = [], 0
    yy, xx = np.mgrid[0:H, 0:W]
    for nc in ncls:
        d = {}
        for n, c in names:
            d[n] = (off, c)
            off += c
        d['heatmap'] = (off, nc)
        hm = buf[:, off:off + nc]
        hm[:] = hm * 0.5 - 4.0
        for b in range(B):
            for _ in range(n_obj):
                c, y, x = g.integers(nc), g.integers(H), g.integers(W)
                hm[b, c] += 6.5 * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * g.uniform(1.0, 6.0)))
        off += nc
        preds.append(d)
    return buf, preds


def maps(B, dev, seed=256, shrink=False):
    """shrink: log-extents of -20 (boxes of 2e-9 m: no two circumscribed circles meet)."""
    buf, layout = fake_preds(B, H, W, seed)
    if shrink:
        for d in layout:
            o, c = d['dim']
            buf[:, o:o + c] = -20.0
    dbuf = torch.from_numpy(buf).to(dev)
    return tuple([{k: dbuf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)


def device_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernel_stats(path):
    """Average µs per call of the decode kernels in a `rocprofv3 --kernel-trace --stats` kernel_stats.csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k + '<' in row['Name'] or k + '(' in row['Name']:
                    calls, total = int(row['Calls']), float(row['TotalDurationNs'])
                    c0, t0 = out.get(k, (0, 0.0))
                    out[k] = (c0 + calls, t0 + total)
    return {k: dict(calls=c, avg_us=round(t / c / 1e3, 2)) for k, (c, t) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile', action='store_true', help='only a few decodes of each type at --batch, for rocprofv3')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--kernel-stats', action='append', default=[], metavar='BATCH=CSV',
                    help='kernel_stats.csv of a --profile run under rocprofv3, folded into the JSON line')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device('cuda:0')
    hd = heads()
    if args.profile:
        preds = maps(args.batch, dev)
        for _ in range(20):
            for kind in ('circle', 'rotate'):
                hd[kind].decode_device(preds)
        torch.cuda.synchronize()
        print("profile run done")
        return
    res = dict(maps=dict(tasks=6, h=H, w=W, max_num=500, blobs_per_task=40), iters=args.iters, rounds=args.rounds)
    for B in (1, 8):
        preds = {k: maps(B, dev, shrink='noclip' in k) for k in KINDS}
        counts = {}
        for kind in KINDS:
            for _ in range(10):                                   # warm-up: code objects, the allocator's blocks
                packed = hd[kind].decode_device(preds[kind])
            counts[kind] = hd[kind].decode_views(packed, B)[3].tolist()
        us = {k: [] for k in KINDS}
        for _ in range(args.rounds):
            for kind in KINDS:
                us[kind].append(device_us(lambda: hd[kind].decode_device(preds[kind]), args.iters))
        r = {}
        for kind in KINDS:
            r[kind] = dict(us_per_call=round(statistics.median(us[kind]), 1), min=round(min(us[kind]), 1), max=round(max(us[kind]), 1),
                           detections_per_sample=counts[kind])
        r['rotate_over_circle'] = round(r['rotate']['us_per_call'] / r['circle']['us_per_call'], 3)
        res[f'b{B}'] = r
    for spec in args.kernel_stats:
        b, path = spec.split('=', 1)
        res.setdefault(f'b{int(b)}', {})['kernel_avg_us_under_rocprofv3'] = kernel_stats(path)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
