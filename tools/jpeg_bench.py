"""On-device JPEG decoding (csrc/jpeg.hip) on synthetic 1080x1920 4:2:0 camera files of 200-350 KB, without and with a
restart marker per MCU row: µs per frame at batch 1 / 4 / 8 from HIP events after warm-up (the upload of the packed
scans included; the host parse + pack timed separately), decode + ImagePreprocessor per frame, the subsequence length
swept at batch 8, and Pillow's one-thread CPU decode for context.  Prints one JSON line (kept as
profiles/jpeg_bench.json).

    python tools/jpeg_bench.py [--iters 20] [--out profiles/jpeg_bench.json]   # the measurement
    python tools/jpeg_bench.py --profile       # only batch-8 decodes, for `rocprofv3 --kernel-trace --stats`
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_jpeg import encode, scene  # noqa: E402

from sgv3d_amd.jpeg import JpegDecoder  # noqa: E402
from sgv3d_amd.preprocess import ImagePreprocessor  # noqa: E402

HW = (1080, 1920)
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)


def files(n, restart):
    kw = dict(quality=72, subsampling=2)
    if restart:
        kw['restart_marker_rows'] = 1
    out = [encode(scene(HW[0], HW[1], 200 + i), **kw) for i in range(n)]
    assert all(200_000 <= len(f) <= 350_000 for f in out), [len(f) for f in out]
    return out


def device_us(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def pillow_ms(data, reps=10):
    from PIL import Image
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(data)))
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    plain, rst = files(8, False), files(8, True)
    dec = JpegDecoder(HW, max_bytes=1 << 19, device=dev)
    if args.profile:
        for fs in (plain, rst):
            for _ in range(5):
                dec(fs)
        torch.cuda.synchronize()
        print("profile run done")
        return
    res = dict(frame_hw=list(HW), sampling='4:2:0', max_bytes=dec.max_bytes, seq_bytes=dec.seq_bytes,
               file_kb={'plain': [round(len(f) / 1e3, 1) for f in plain], 'restart_rows': [round(len(f) / 1e3, 1) for f in rst]})
    pre = ImagePreprocessor({'final_dim': (864, 1536), 'bot_pct_lim': (0.0, 0.0)}, IMG_CONF, src_hw=HW, device=dev)
    for tag, fs in (('plain', plain), ('restart_rows', rst)):
        r = {}
        for b in (1, 4, 8):
            batch = fs[:b]
            out = dec(batch)
            assert dec.status().tolist() == [0] * b
            r[f'b{b}_us_per_frame'] = round(device_us(lambda: dec(batch, out=out), args.iters) / b, 1)
            r[f'b{b}_decode_preprocess_us_per_frame'] = round(
                device_us(lambda: pre(dec(batch, out=out)), args.iters) / b, 1)
            t = time.perf_counter()
            for _ in range(args.iters):
                recs, scans, _ = dec.plan(batch)
                dec.pack(recs, scans, np.empty(dec.packed_bytes(scans), np.uint8))
            r[f'b{b}_host_parse_pack_us_per_frame'] = round((time.perf_counter() - t) * 1e6 / args.iters / b, 1)
        sweep = {}
        for seq in (16, 32, 64, 128, 256, 1024):
            out = dec(fs, seq_bytes=seq)
            assert dec.status().tolist() == [0] * 8
            sweep[str(seq)] = round(device_us(lambda: dec(fs, out=out, seq_bytes=seq), args.iters) / 8, 1)
        r['b8_us_per_frame_by_seq_bytes'] = sweep
        best, med = pillow_ms(fs[0])
        r['pillow_1thread_ms'] = dict(best=round(best, 2), median=round(med, 2))
        r['speedup_b8_vs_pillow_best'] = round(best * 1e3 / r['b8_us_per_frame'], 1)
        res[tag] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
