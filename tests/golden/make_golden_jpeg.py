"""Regenerates tests/golden/jpeg.npz and jpeg_stress.npz: JPEG files written by Pillow from seeded synthetic images (and
re-coded by tests/jpeg_recode.py), with Pillow's decode.

    python tests/golden/make_golden_jpeg.py

Small cases (``<name>_jpg`` the file's bytes, ``<name>_rgb`` np.asarray(Image.open(file))): 4:2:0, 4:2:2 and 4:4:4 at
odd sizes, restart intervals of 1 and 7 MCUs, optimised Huffman tables, quality 100 and 5.  Two 1080x1920 4:2:0 files of
200-350 KB without and with a restart marker per MCU row, whose decode is kept as a CRC32 per row (``<name>_crc``).
Files the decoder must reject (``bad_<what>``): progressive, grayscale, CMYK, truncated inside the scan, and SOF headers
patched to arithmetic coding and to 12-bit samples.  Pillow and numpy only.  A committed jpeg.npz is never rewritten:
the regenerated arrays are compared with it and the outcome is printed.

jpeg_stress.npz holds valid files that are hard on a decoder (``<name>_jpg``; Pillow's decode of exactly those bytes as
``<name>_rgb``, as ``<name>_crc`` for frames above 128 KB of pixels, or as an entry ``<name>=<other>`` of ``same``: the
case whose ``_rgb`` Pillow's decode of this file equals byte for byte (asserted here), so that restart and re-coded
variants of one image share one copy of the pixels):

* ``sw<sampling>_<h>x<w>``: every width of SWEEP at height 17 and every height of SWEEP at width 33, ``scene`` with
  saturated patches on the right and bottom edges;
* ``cc<sampling>_<class>_r<interval>`` at 64x96 and ``cx420_<class>_r<interval>`` at 256x256: the content classes of
  ``CLASSES`` (noise at quality 100, that is with all-ones tables, and with three different quantisation tables (the
  noise cases take a subset of the intervals and one 256x256 file: they do not compress), a constant colour, 8x8
  black and white blocks, a one-pixel checkerboard, sparse high frequencies that need ZRL symbols);
* ``rc_<source>_<variant>``: four sources re-coded with long, edge9 and split Huffman tables, fill bytes, other restart
  intervals, extra segments and one segment per table (asserted here: Pillow decodes each to its source's pixels);
* ``big_*``: a 1024x1040 4:2:0 frame (more luma blocks than one DC chunk, 65 MCUs per row, restart interval 7), the same
  with long tables, and a 2176x3840 frame.
The file is written with fixed zip time stamps: two runs give the same bytes.
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def scene(h, w, seed):
    """A seeded synthetic camera-like frame: smooth shading, flat patches with edges, blocky texture, sensor noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 3), np.float32)
    for c in range(3):
        img[..., c] = 110 + 60 * np.sin(x / (w / rng.uniform(1, 4)) + rng.uniform(0, 6)) * np.cos(y / (h / rng.uniform(1, 3)))
    for _ in range(40):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        img[y0:y0 + rng.integers(4, h // 3 + 5), x0:x0 + rng.integers(4, w // 3 + 5)] = rng.uniform(0, 255, 3)
    small = rng.normal(0, 1, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    img += 25 * np.kron(small, np.ones((8, 8, 1), np.float32))[:h, :w]
    img += rng.normal(0, 6, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', **kw)
    return b.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def row_crc(rgb):
    return np.array([zlib.crc32(r.tobytes()) for r in rgb], np.uint32)


SMALL = {   # name: (h, w, seed, save options)
    's420_61x83': (61, 83, 1, dict(quality=85, subsampling=2)),
    's422_61x83': (61, 83, 2, dict(quality=85, subsampling=1)),
    's444_61x83': (61, 83, 3, dict(quality=85, subsampling=0)),
    's420_17x9': (17, 9, 4, dict(quality=90, subsampling=2)),
    's422_17x9': (17, 9, 5, dict(quality=90, subsampling=1)),
    's444_8x8': (8, 8, 6, dict(quality=90, subsampling=0)),
    's420_1x1': (1, 1, 7, dict(quality=90, subsampling=2)),
    'rst1': (61, 83, 8, dict(quality=80, subsampling=2, restart_marker_blocks=1)),
    'rst7': (61, 83, 9, dict(quality=80, subsampling=1, restart_marker_blocks=7)),
    'optimize': (61, 83, 10, dict(quality=80, subsampling=2, optimize=True)),
    'q100': (61, 83, 11, dict(quality=100, subsampling=0)),
    'q5': (61, 83, 12, dict(quality=5, subsampling=2)),
}
FULL = {'full_plain': (21, dict(quality=72, subsampling=2)),
        'full_rst': (22, dict(quality=72, subsampling=2, restart_marker_rows=1))}


def sof_patched(data, marker=None, precision=None):
    b = bytearray(data)
    i = b.index(b'\xff\xc0')
    if marker is not None:
        b[i + 1] = marker
    if precision is not None:
        b[i + 4] = precision
    return bytes(b)


# ---------------------------------------------------------------------------------------------- jpeg_stress.npz
SAMPLING = {'444': 0, '422': 1, '420': 2}
SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49)
SWEEP_SIZES = [(17, w) for w in SWEEP] + [(h, 33) for h in SWEEP if h != 17]


def edge_scene(h, w, seed):
    """``scene`` plus pure red / blue / green / magenta patches that touch the right and the bottom edge."""
    img = scene(h, w, seed)
    rng = np.random.default_rng(seed + 1000)
    cols = np.array([[255, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 255]], np.uint8)
    for i in range(4):
        a, b = int(rng.integers(1, 4)), int(rng.integers(1, 6))
        y0 = int(rng.integers(0, h))
        img[y0:y0 + b, max(0, w - a):] = cols[i]                       # the right edge
        x0 = int(rng.integers(0, w))
        img[max(0, h - a):, x0:x0 + b] = cols[(i + 1) % 4]              # the bottom edge
    img[max(0, h - 1):, max(0, w - 1):] = cols[seed % 4]                # the corner pixel
    return img


def smooth(h, w, seed):
    """Smooth shading with a few flat patches: a small file at any frame size."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 90 * np.sin(x / rng.uniform(150, 400) + rng.uniform(0, 6)) * np.cos(y / rng.uniform(150, 400))
                    for _ in range(3)], -1)
    for _ in range(12):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        img[y0:y0 + rng.integers(20, h // 4), x0:x0 + rng.integers(20, w // 4)] = rng.uniform(0, 255, 3)
    return np.clip(img, 0, 255).astype(np.uint8)


def _zrl(h, w, seed):
    """Grey blocks that hold one or two high-frequency cosines each: long zero runs before the last coefficients."""
    rng = np.random.default_rng(seed)
    n = np.arange(8)
    img = np.full((h, w), 128, np.float32)
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            if rng.random() < 0.3:
                continue
            for _ in range(int(rng.integers(1, 3))):
                u, v = [(7, 7), (7, 6), (6, 7), (5, 7), (7, 3), (0, 7)][int(rng.integers(0, 6))]
                amp = float(rng.uniform(20, 60)) * (1 if rng.random() < 0.5 else -1)
                img[by:by + 8, bx:bx + 8] += amp * np.outer(np.cos((2 * n + 1) * v * np.pi / 16),
                                                            np.cos((2 * n + 1) * u * np.pi / 16))[:h - by, :w - bx]
    return np.repeat(np.clip(img, 0, 255).astype(np.uint8)[..., None], 3, -1)


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _grid(h, w, cell):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y // cell + x // cell) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


QT3 = [[2 + (i % 8) + i // 8 for i in range(64)], [3 + 2 * (i % 8) for i in range(64)],
       [5 + 3 * (i // 8) for i in range(64)]]
CLASSES = {   # name: (image(h, w, seed), save options)
    'noise_q100': (_noise, dict(quality=100)),            # (libjpeg's quality 100 is the all-ones table: one class)
    'noise_q3': (_noise, dict(qtables=QT3)),
    'const': (lambda h, w, seed: np.full((h, w, 3), (200, 30, 90), np.uint8), dict(quality=90)),
    'bw8': (lambda h, w, seed: _grid(h, w, 8), dict(quality=100)),
    'checker': (lambda h, w, seed: _grid(h, w, 1), dict(quality=100)),
    'zrl': (_zrl, dict(quality=90)),
}
# Noise files and their decodes do not compress, and the fixture has a size cap: each restart interval still meets noise
# in every sampling, but not every (class, sampling, interval); the other classes take all four intervals.
NOISE_RESTARTS = {('420', 'noise_q100'): (0, 1, 6), ('422', 'noise_q100'): (1,), ('444', 'noise_q100'): (3,),
                  ('420', 'noise_q3'): (0,), ('422', 'noise_q3'): (3, 6), ('444', 'noise_q3'): (1,)}
RECODE_SOURCES = {   # name: how to make the source file ('noise' has three different quantisation tables)
    'noise': lambda: encode(_noise(64, 96, 301), qtables=QT3, subsampling=2),
    'const': lambda: encode(np.full((64, 96, 3), (200, 30, 90), np.uint8), quality=90, subsampling=2),
    'scene420': lambda: encode(scene(61, 83, 1), quality=85, subsampling=2),
    'scene444': lambda: encode(scene(61, 83, 3), quality=85, subsampling=0),
}
RECODE_VARIANTS = {
    'long': dict(tables='long'), 'edge9': dict(tables='edge9'), 'split': dict(tables='split'),
    'fill1': dict(fill=1, restart=2), 'fill3': dict(fill=3, restart=2), 'r5': dict(restart=5),
    'seg': dict(segments='extra'), 'each': dict(segments='each'),
    'combo': dict(tables='split', restart=3, fill=2, segments='extra each'),
}


def restart_kw(ri):
    return dict(restart_marker_blocks=ri) if ri else {}


def stress_cases():
    """-> {array name: array} of jpeg_stress.npz."""
    sys.path.insert(0, os.path.dirname(HERE))
    from jpeg_recode import recode
    out, alias = {}, []

    def put(name, data, same=None):
        rgb = pil_decode(data)
        out[f'{name}_jpg'] = np.frombuffer(data, np.uint8)
        if same is not None:
            assert np.array_equal(rgb, same[1]), f"{name}: Pillow's decode differs from {same[0]}"
            alias.append(f'{name}={same[0]}')
        elif rgb.size > 128 * 1024:
            out[f'{name}_crc'] = row_crc(rgb)
        else:
            out[f'{name}_rgb'] = rgb
        return rgb

    for si, (sname, sub) in enumerate(SAMPLING.items()):
        for i, (h, w) in enumerate(SWEEP_SIZES):
            put(f'sw{sname}_{h}x{w}', encode(edge_scene(h, w, 400 + 40 * si + i), quality=90, subsampling=sub))
    for si, (sname, sub) in enumerate(SAMPLING.items()):
        row = 96 // (8 if sub == 0 else 16)
        for ci, (cname, (make, kw)) in enumerate(CLASSES.items()):
            img = make(64, 96, 300 + 10 * si + ci)
            first = None
            for ri in NOISE_RESTARTS.get((sname, cname), (0, 1, 3, row)):
                name = f'cc{sname}_{cname}_r{ri}'
                rgb = put(name, encode(img, subsampling=sub, **kw, **restart_kw(ri)), first)
                first = first or (name, rgb)
    for ci, (cname, (make, kw)) in enumerate(CLASSES.items()):
        img = make(256, 256, 350 + ci)
        if cname == 'noise_q3':
            continue
        kw = dict(kw, quality=75) if cname == 'noise_q100' else kw      # (the size cap again)
        for ri in ((1,) if cname == 'noise_q100' else (0, 1, 5)):
            put(f'cx420_{cname}_r{ri}', encode(img, subsampling=2, **kw, **restart_kw(ri)))
    for sname, make in RECODE_SOURCES.items():
        src = make()
        rgb = put(f'rc_{sname}_src', src)
        for vname, kw in RECODE_VARIANTS.items():
            if (sname, vname) == ('noise', 'each'):   # (the size cap; 'combo' writes one segment per table too)
                continue
            put(f'rc_{sname}_{vname}', recode(src, **kw), (f'rc_{sname}_src', rgb))
    big = encode(smooth(1024, 1040, 40), quality=10, subsampling=2, restart_marker_blocks=7)
    put('big_1024x1040_r7', big)
    long_ = recode(big, tables='long')
    assert np.array_equal(pil_decode(long_), pil_decode(big))
    put('big_1024x1040_r7_long', long_)
    put('big_2176x3840', encode(smooth(2176, 3840, 41), quality=5, subsampling=2))
    out['same'] = np.array(alias)
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED, compresslevel=9)


def main():
    out = {}
    for name, (h, w, seed, kw) in SMALL.items():
        data = encode(scene(h, w, seed), **kw)
        out[f'{name}_jpg'] = np.frombuffer(data, np.uint8)
        out[f'{name}_rgb'] = pil_decode(data)
    for name, (seed, kw) in FULL.items():
        data = encode(scene(1080, 1920, seed), **kw)
        assert 200_000 <= len(data) <= 350_000, (name, len(data))
        out[f'{name}_jpg'] = np.frombuffer(data, np.uint8)
        out[f'{name}_crc'] = row_crc(pil_decode(data))
    img = scene(32, 48, 30)
    base = encode(img, quality=80)
    bad = {
        'progressive': encode(img, quality=80, progressive=True),
        'grayscale': encode(img[..., 0].copy(), quality=80),
        'cmyk': (lambda b: (Image.fromarray(img).convert('CMYK').save(b, 'JPEG', quality=80), b.getvalue())[1])(io.BytesIO()),
        'truncated': base[:len(base) - 64],   # inside the scan
        'arithmetic': sof_patched(base, marker=0xC9),
        '12bit': sof_patched(base, precision=12),
    }
    for k, v in bad.items():
        out[f'bad_{k}'] = np.frombuffer(v, np.uint8)
    path = os.path.join(HERE, 'jpeg.npz')
    if os.path.exists(path):   # the committed file stays as it is; say whether this Pillow reproduces it
        old = np.load(path)
        same = sorted(old.files) == sorted(out) and all(np.array_equal(old[k], out[k]) for k in out)
        print(path, 'reproduced, left unchanged' if same else 'NOT reproduced by this Pillow, left unchanged')
    else:
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), 'bytes')
    path = os.path.join(HERE, 'jpeg_stress.npz')
    write_npz(path, stress_cases())
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
