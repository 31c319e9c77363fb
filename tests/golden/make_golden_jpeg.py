"""Regenerates tests/golden/jpeg.npz: JPEG files written by Pillow from seeded synthetic images, with Pillow's decode.

    python tests/golden/make_golden_jpeg.py

Small cases (``<name>_jpg`` the file's bytes, ``<name>_rgb`` np.asarray(Image.open(file))): 4:2:0, 4:2:2 and 4:4:4 at
odd sizes, restart intervals of 1 and 7 MCUs, optimised Huffman tables, quality 100 and 5.  Two 1080x1920 4:2:0 files of
200-350 KB without and with a restart marker per MCU row, whose decode is kept as a CRC32 per row (``<name>_crc``).
Files the decoder must reject (``bad_<what>``): progressive, grayscale, CMYK, truncated inside the scan, and SOF headers
patched to arithmetic coding and to 12-bit samples.  Pillow and numpy only.
"""
import io
import os
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
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
