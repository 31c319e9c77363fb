"""Time the preprocessing launch (csrc/preprocess.hip) at the shipped DAIR size, 1080x1920 uint8 frames -> 864x1536 float32,
and print one JSON line.

Per batch size: microseconds per frame from HIP events around `--iters` back-to-back launches after `--warmup` launches,
the bytes the algorithm has to move (uint8 frames in, float32 planes out) and their rate as a fraction of 8 TB/s.  For
context, the reference's CPU path for one frame (PIL bicubic resize + crop, then the numpy normalise and CHW transpose of
mmcv.imnormalize; one thread) when Pillow is importable.

    python tools/preprocess_bench.py [--batches 1 4 8] [--iters 200] [--out profiles/preprocess_bench.json]
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

from sgv3d_amd.preprocess import ImagePreprocessor  # noqa: E402

HBM_PEAK = 8.0e12
SRC_HW, FINAL = (1080, 1920), (864, 1536)
IDA_AUG_CONF = {'final_dim': FINAL, 'bot_pct_lim': (0.0, 0.0)}
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)


def gpu_rows(batches, iters, warmup):
    assert torch.cuda.is_available(), "preprocess_bench needs the GPU"
    dev = torch.device('cuda', 0)
    pre = ImagePreprocessor(IDA_AUG_CONF, IMG_CONF, src_hw=SRC_HW, device=dev)
    rows = []
    for b in batches:
        frames = torch.randint(0, 256, (b,) + SRC_HW + (3,), dtype=torch.uint8, device=dev)
        out = torch.empty((b, 1, 1, 3) + FINAL, dtype=torch.float32, device=dev)
        for _ in range(warmup):
            pre(frames, out=out)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            pre(frames, out=out)
        t1.record()
        t1.synchronize()
        us_frame = t0.elapsed_time(t1) * 1e3 / (iters * b)
        nbytes = b * (SRC_HW[0] * SRC_HW[1] * 3 + 3 * FINAL[0] * FINAL[1] * 4)
        rows.append({'batch': b, 'us_per_frame': round(us_frame, 3), 'us_per_launch': round(us_frame * b, 3),
                     'bytes_per_launch': nbytes, 'TBps': round(nbytes / (us_frame * b * 1e-6) / 1e12, 3),
                     'fraction_of_8TBps': round(nbytes / (us_frame * b * 1e-6) / HBM_PEAK, 3)})
    return rows


def cpu_row(reps=5):
    try:
        from PIL import Image
    except ImportError:
        return None
    pre = ImagePreprocessor(IDA_AUG_CONF, IMG_CONF, src_hw=SRC_HW, device='cpu')
    src = np.random.default_rng(0).integers(0, 256, SRC_HW + (3,), dtype=np.uint8)
    mean = np.asarray(IMG_CONF['img_mean'], np.float32).reshape(1, 1, 3)
    stdinv = (1.0 / np.asarray(IMG_CONF['img_std'], np.float32).astype(np.float64)).astype(np.float32).reshape(1, 1, 3)
    t_resize, t_norm = [], []
    for _ in range(reps):
        t = time.perf_counter()
        img = np.array(Image.fromarray(src).resize(pre.resize_dims).crop(pre.crop))
        t_resize.append(time.perf_counter() - t)
        t = time.perf_counter()
        x = img.astype(np.float32)[..., ::-1]
        np.ascontiguousarray(((x - mean) * stdinv).transpose(2, 0, 1))
        t_norm.append(time.perf_counter() - t)
    return {'pil_resize_crop_ms': round(1e3 * min(t_resize), 2), 'numpy_normalize_chw_ms': round(1e3 * min(t_norm), 2),
            'threads': 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4, 8])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    torch.set_num_threads(1)
    res = {'metric': 'preprocess 1080x1920 u8 -> 864x1536 f32 (resize + crop + swap + normalise)',
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
