"""Time the training-time augmentation launches (csrc/augment.hip) at the shipped DAIR size, 1080x1920 uint8 frames ->
864x1536 float32, and print one JSON line.

Per setting and batch size: microseconds per frame from HIP events around `--iters` back-to-back calls after `--warmup`
calls (each call: the host plan, one pinned upload, the launches).  Settings: every frame rectified and jittered
('all'), none of them ('none'), and the reference's sampled mix ('sampled': p = 0.5 rectified, 0.3 jittered).  The bytes
are the minimum each stage has to move (uint8 frames through the rectification's passes, the eval resize's passes, the
float32 planes out) and their rate as a fraction of 8 TB/s.  For context, the single-thread CPU cost of the reference's
Pillow part for one frame (LANCZOS resize, paste, BICUBIC rotate) when Pillow is importable.

    python tools/augment_bench.py [--batches 1 4 8] [--iters 50] [--out profiles/augment_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgv3d_amd.train_augment import AugmentParams, TrainAugmenter, sample_params  # noqa: E402

HBM_PEAK = 8.0e12
SRC_HW, FINAL = (1080, 1920), (864, 1536)
IDA_AUG_CONF = {'final_dim': FINAL, 'bot_pct_lim': (0.0, 0.0)}
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)
CENTER = (940, 567)                                  # the DAIR principal point, truncated


def params(setting, n, seed=0):
    if setting == 'sampled':
        p = sample_params(n, random.Random(seed), np.random.RandomState(seed))
        p.center[:] = CENTER
        p.transform_pitch[:] = np.random.RandomState(seed + 1).randint(-30, 31, n)
        p._placed[:] = True
        return p
    on = setting == 'all'
    rs = np.random.RandomState(seed)
    return AugmentParams([on] * n, 1.0 + 0.2 * rs.randn(n) if on else [1.0] * n, 2.0 * rs.randn(n), 0.67 * rs.randn(n),
                         [on] * n, rs.rand(n), center=[CENTER] * n, transform_pitch=rs.randint(-30, 31, n))


def min_bytes(p):
    H, W = SRC_HW
    src, fin = H * W * 3, FINAL[0] * FINAL[1] * 3
    total = 0
    for i in range(len(p)):
        b = src                                       # frame in
        if p.ie[i]:
            b += 6 * src                              # Lanczos h (out + in), v (out + in), warp (out)
        b += int(src * FINAL[1] / W) * 2 + fin        # eval resize: h pass out + in, v pass out (uint8)
        b += fin + 4 * fin                            # normalise: uint8 in, float32 out
        total += b
    return total


def gpu_rows(batches, iters, warmup):
    assert torch.cuda.is_available(), "augment_bench needs the GPU"
    dev = torch.device('cuda', 0)
    aug = TrainAugmenter(IDA_AUG_CONF, IMG_CONF, src_hw=SRC_HW, device=dev)
    rows = []
    for setting in ('all', 'none', 'sampled'):
        for b in batches:
            frames = torch.randint(0, 256, (b,) + SRC_HW + (3,), dtype=torch.uint8, device=dev)
            p = params(setting, b, seed=b)
            for _ in range(warmup):
                aug(frames, p)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                aug(frames, p)
            t1.record()
            t1.synchronize()
            us_frame = t0.elapsed_time(t1) * 1e3 / (iters * b)
            nbytes = min_bytes(p)
            rows.append({'setting': setting, 'batch': b, 'rectified': int(p.ie.sum()), 'jittered': int(p.bright.sum()),
                         'us_per_frame': round(us_frame, 3), 'us_per_call': round(us_frame * b, 3),
                         'min_bytes_per_call': nbytes,
                         'fraction_of_8TBps': round(nbytes / (us_frame * b * 1e-6) / HBM_PEAK, 3)})
    return rows


def cpu_row(reps=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    H, W = SRC_HW
    src = Image.fromarray(np.random.default_rng(0).integers(0, 256, SRC_HW + (3,), dtype=np.uint8))
    ratio, roll, tp = 0.9, 1.5, 12
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        img = src.resize((int(W * ratio), int(H * ratio)), Image.LANCZOS)
        canvas = Image.new(mode='RGB', size=(W, H))
        w_min, h_min = int(CENTER[0] * (1 - ratio)), int(CENTER[1] * (1 - ratio))
        canvas.paste(img, (w_min, h_min, w_min + img.size[0], h_min + img.size[1]))
        canvas.rotate(-roll, center=CENTER, translate=(0, tp), fillcolor=(0, 0, 0), resample=Image.BICUBIC)
        ts.append(time.perf_counter() - t)
    return {'pil_lanczos_paste_rotate_ms': round(1e3 * min(ts), 2), 'threads': 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4, 8])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    torch.set_num_threads(1)
    res = {'metric': 'train augmentation 1080x1920 u8 -> 864x1536 f32 (rectify + resize + crop + brightness + normalise)',
           'device': torch.cuda.get_device_name(0), 'gpu': gpu_rows(a.batches, a.iters, a.warmup),
           'cpu_one_frame': None if a.no_cpu else cpu_row()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
