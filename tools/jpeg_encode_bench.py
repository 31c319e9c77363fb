"""On-device JPEG encoding (csrc/jpeg_encode.hip) on synthetic 1080x1920 camera frames (the scenes of
tests/golden/make_golden_jpeg.py): quality 95 and 75, 4:2:0, without restart markers and with one per MCU row, batch 1 and
8.  HIP events around ``enc(frames)`` + ``.files()`` (the seven launches and both copies to the host), median of 10 after
warm-up; the launches alone; Pillow's one-thread ``save`` of the same frames in the same run where Pillow is importable
(otherwise the figure is absent and ``pillow`` says so); and ``JpegDecoder`` on the encoder's own files with and without
restart markers.  Every file is checked against ``sgv3d_jpeg_encode_host`` for the first frame.  Prints one JSON line (kept
as profiles/jpeg_encode_bench.json).

    python tools/jpeg_encode_bench.py [--out profiles/jpeg_encode_bench.json]   # the measurement
    python tools/jpeg_encode_bench.py --profile       # only batch-8 encodes, for `rocprofv3 --kernel-trace --stats`
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
from make_golden_jpeg import scene  # noqa: E402

from sgv3d_amd import _lib  # noqa: E402
from sgv3d_amd.jpeg import JpegDecoder  # noqa: E402
from sgv3d_amd.jpeg_encode import JpegEncoder  # noqa: E402

HW = (1080, 1920)
MCU_ROW = 120           # MCUs per row of a 1920-wide 4:2:0 frame


def median_ms(fn, reps=10, warm=3):
    """HIP events around fn (which ends with the host holding the result), median of reps after warm-up."""
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


def pillow_ms(frames, quality, restart, reps=10):
    """One-thread Pillow: ms per frame, the median over reps of the mean over the frames."""
    from PIL import Image
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        for f in frames:
            Image.fromarray(f).save(io.BytesIO(), format='JPEG', quality=quality, subsampling='4:2:0', restart_marker_blocks=restart)
        ts.append((time.perf_counter() - t) * 1e3 / len(frames))
    return statistics.median(ts)


def host_file(frame, quality, restart, max_bytes):
    lib = _lib.load()
    files, ln, st = np.zeros((max_bytes + 15) // 16 * 16, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32)
    frame = np.ascontiguousarray(frame)
    rc = lib.sgv3d_jpeg_encode_host(1, HW[0], HW[1], quality, 2, 2, restart, max_bytes, frame.ctypes.data, files.ctypes.data, files.size,
                                    ln.ctypes.data, st.ctypes.data)
    assert rc == 0 and st[0] == 0
    return files[:ln[0]].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    host = np.stack([scene(HW[0], HW[1], 300 + i) for i in range(8)])
    frames = torch.from_numpy(host).to(dev)
    if args.profile:
        enc = JpegEncoder(HW, quality=95, restart=MCU_ROW, device=dev)
        for _ in range(5):
            enc(frames).files()
        print("profile run done")
        return
    try:
        import PIL
        pillow = f"Pillow {PIL.__version__}, one thread, the same frames in this run"
    except ImportError:
        pillow = None
    res = dict(frame_hw=list(HW), sampling='4:2:0', input='synthetic scenes (tests/golden/make_golden_jpeg.py)',
               method='HIP events around enc(frames) + .files(), median of 10 after 3 warm-up calls',
               pillow=pillow or 'not importable here: no baseline in this run')
    files_for_decode = {}
    for quality in (95, 75):
        for restart in (0, MCU_ROW):
            enc = JpegEncoder(HW, quality=quality, restart=restart, device=dev)
            r = dict(max_bytes=enc.max_bytes)
            for b in (1, 8):
                batch = frames[:b]
                n = enc.workspace_bytes(b)
                work = torch.empty(n, dtype=torch.uint8, device=dev)
                out = torch.empty(b * enc.slot_bytes, dtype=torch.uint8, device=dev)
                words = torch.empty(2 * b, dtype=torch.int32, device=dev)
                got = enc(batch, work=work, files=out, words=words).files()
                if b == 1:
                    assert got[0] == host_file(host[0], quality, restart, enc.max_bytes), "the kernels differ from the host entry"
                    r['file_kb'] = round(len(got[0]) / 1e3, 1)
                total = median_ms(lambda: enc(batch, work=work, files=out, words=words).files())
                launches = median_ms(lambda: (enc(batch, work=work, files=out, words=words), torch.cuda.synchronize()))
                r[f'b{b}_ms_per_frame_with_copies'] = round(total / b, 3)
                r[f'b{b}_ms_per_frame_launches_only'] = round(launches / b, 3)
                if b == 8:
                    files_for_decode[(quality, restart)] = got
            if pillow:
                r['pillow_ms_per_frame'] = round(pillow_ms(host, quality, restart), 2)
                r['b8_speedup_vs_pillow'] = round(r['pillow_ms_per_frame'] / r['b8_ms_per_frame_with_copies'], 1)
                r['b1_speedup_vs_pillow'] = round(r['pillow_ms_per_frame'] / r['b1_ms_per_frame_with_copies'], 1)
            res[f'q{quality}_restart{restart}'] = r
    dec = JpegDecoder(HW, max_bytes=1 << 21, device=dev)
    out = torch.empty(8, HW[0], HW[1], 3, dtype=torch.uint8, device=dev)
    for (quality, restart), fs in files_for_decode.items():
        dec(fs, out=out)
        assert dec.status().tolist() == [0] * 8
        ms = median_ms(lambda: (dec(fs, out=out), torch.cuda.synchronize()))
        res[f'q{quality}_restart{restart}']['b8_decode_of_these_files_ms_per_frame'] = round(ms / 8, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
