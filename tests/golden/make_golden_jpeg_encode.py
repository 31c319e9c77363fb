"""Writes tests/golden/jpeg_encode.npz: uint8 frames and the files Pillow (libjpeg-turbo) encodes them to.

    python tests/golden/make_golden_jpeg_encode.py

Every case is ``Image.fromarray(frame).save(f, format='JPEG', quality=q, subsampling=s, restart_marker_blocks=r)``.  The
script asserts with tests/jpeg_ref.py that the set holds the corners the encoder's tests rely on: a DC difference of 11
bits, an AC value of 10 bits, a non-zero coefficient 63, a ZRL, stuffed FF 00 bytes and a file larger than its raw frame.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as R  # noqa: E402

SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 33), (24, 40), (24, 48), (40, 24), (37, 61), (41, 65), (130, 260), (168, 328)]
CONTENTS = ['noise', 'smooth', 'zeros', 'ones', 'blocks', 'stripes', 'checker']
SUBS = ['4:4:4', '4:2:2', '4:2:0']
MCU = {'4:4:4': (8, 8), '4:2:2': (8, 16), '4:2:0': (16, 16)}     # (rows, columns) of an MCU


def content(kind, h, w, rng):
    yy, xx = np.mgrid[:h, :w]
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'smooth':
        ramp = np.stack([yy * 2 + xx, 255 - xx * 3, yy * 3 + 20], -1) % 256
        return np.clip(ramp + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    gray = {'zeros': np.zeros((h, w)), 'ones': np.full((h, w), 255), 'blocks': ((yy // 8 + xx // 8) & 1) * 255,
            'stripes': (xx & 1) * 255, 'checker': ((yy + xx) & 1) * 255}[kind]
    return np.repeat(gray.astype(np.uint8)[:, :, None], 3, axis=2)


def mcus(h, w, sub):
    mh, mw = MCU[sub]
    return -(-w // mw), -(-h // mh)


def main():
    rng = np.random.default_rng(20261019)
    inputs, cases = {}, []

    def add(h, w, kind, sub, q, r):
        key = f"in_{h}x{w}_{kind}"
        if key not in inputs:
            inputs[key] = np.ascontiguousarray(content(kind, h, w, rng))
        name = f"{h}x{w}_{kind}_{sub.replace(':', '')}_q{q}_r{r}"
        if name not in [c[0] for c in cases]:
            cases.append((name, h, w, kind, sub, q, r))

    qs = [10, 30, 75, 95, 100]
    small = SIZES[:10]
    for i, (h, w) in enumerate(small):                            # every small size at every sampling, qualities in turn
        for j, sub in enumerate(SUBS):
            add(h, w, 'noise', sub, qs[(i + j) % 5], 0)
        add(h, w, 'smooth', '4:2:0', 95, 1)
    for h, w in [(24, 40), (24, 48), (40, 24), (37, 61)]:          # dummy blocks and the chroma bottom rule, every content
        for kind in CONTENTS:
            add(h, w, kind, '4:2:0', 75, 0)
        add(h, w, 'smooth', '4:2:2', 75, 0)
        add(h, w, 'smooth', '4:4:4', 75, 0)
    for sub in SUBS:                                               # a non-zero coefficient 63; 11-bit DC; 10-bit AC; FF 00
        add(37, 61, 'noise', sub, 100, 0)
        for kind in ('blocks', 'stripes', 'checker', 'zeros', 'ones'):
            add(37, 61, kind, sub, 100, 0)
    add(37, 61, 'noise', '4:2:0', 30, 5)                           # 12 MCUs: 5 does not divide them
    add(37, 61, 'noise', '4:2:0', 75, 3)
    add(37, 61, 'noise', '4:2:0', 75, mcus(37, 61, '4:2:0')[0])    # one MCU row
    add(41, 65, 'noise', '4:2:0', 75, 1)                           # 15 intervals: RST7 wraps to RST0
    add(41, 65, 'checker', '4:4:4', 95, 1)                         # 54 intervals
    add(41, 65, 'smooth', '4:4:4', 95, mcus(41, 65, '4:4:4')[0])
    add(41, 65, 'noise', '4:2:2', 10, 5)
    add(130, 260, 'noise', '4:2:0', 30, 0)                         # ZRLs
    add(130, 260, 'noise', '4:2:2', 75, mcus(130, 260, '4:2:2')[0])
    add(130, 260, 'smooth', '4:2:0', 95, 0)
    add(130, 260, 'noise', '4:4:4', 100, 0)                        # larger than the raw frame
    add(130, 260, 'checker', '4:2:0', 100, 3)
    add(168, 328, 'noise', '4:2:0', 75, 0)                         # no multiple of any chunk the kernels use: 1386 blocks
    add(168, 328, 'smooth', '4:2:0', 95, mcus(168, 328, '4:2:0')[0])
    add(168, 328, 'stripes', '4:2:2', 75, 7)

    files, seen = {}, dict(dc11=0, ac10=0, c63=0, zrl=0, ff00=0, larger=0)
    for name, h, w, kind, sub, q, r in cases:
        buf = io.BytesIO()
        Image.fromarray(inputs[f"in_{h}x{w}_{kind}"]).save(buf, format='JPEG', quality=q, subsampling=sub, restart_marker_blocks=r)
        data = buf.getvalue()
        files[f"f_{name}"] = np.frombuffer(data, np.uint8)
        info = R.parse(data)
        seen['ff00'] += info['scan'].count(b'\xff\x00')
        seen['larger'] += len(data) > h * w * 3
        if h * w <= 65 * 65:                                       # (the restatement's decoder reads bit by bit)
            trace = []
            coef = R.coefficients(info, trace)
            seen['dc11'] += sum(1 for c, _, s in trace if c == 0 and s == 11)
            seen['ac10'] += sum(1 for c, _, s in trace if c == 1 and (s & 15) == 10)
            seen['zrl'] += sum(1 for c, _, s in trace if c == 1 and s == 0xF0)
            seen['c63'] += int(np.count_nonzero(coef[:, 63]))
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    lines = np.array(['|'.join(str(v) for v in c) for c in cases])
    path = os.path.join(HERE, 'jpeg_encode.npz')
    np.savez_compressed(path, cases=lines, **inputs, **files)
    print(f"{len(cases)} cases, {len(inputs)} inputs, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
