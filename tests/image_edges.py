"""The case table of tests/golden/image_edges.npz (test helper, shared by its maker tests/golden/make_golden_image_edges.py
and by tests/test_image_edges_cpu.py / _gpu.py): resize geometries that reach every tap-count template of
csrc/preprocess.hip, its large-LDS path and both of its scalar store tails, the crop boxes that hang over each side of the
resized image, and the launch's LDS formula restated so that the tests can say which path a case takes."""
import math
import os

import numpy as np

# name: (source (H, W), resized (H, W), content, (kx, ky), crop boxes and flips as well?)
CASES = {
    'kt9': ((61, 83), (31, 42), 'noise', (9, 9), True),            # a downscale in (1.5, 2]: the KT = 9 template
    'ks13_steps': ((67, 90), (23, 31), 'steps', (13, 13), False),  # ksize 13, both clamps of clip8 in both passes
    'ks17_4x': ((64, 132), (16, 33), 'checker', (17, 17), False),  # exact 4.0x: ksize 17, 86 560 B of LDS
    'ks17_3p9x': ((67, 131), (17, 33), 'noise', (17, 17), True),   # ksize 17, 85 520 B of LDS
    'aniso_a': ((90, 40), (30, 100), 'steps', (5, 13), False),     # kx != ky: upscale across, 3x down
    'aniso_b': ((20, 260), (33, 65), 'checker', (17, 5), True),    # one column past a 64-tile, one row past two 16-tiles
    'identity': ((37, 53), (37, 53), 'noise', (5, 5), True),       # identity coefficients, crop only
    'one_pixel': ((1, 1), (1, 1), 'white', (5, 5), False),
    'one_col_up': ((9, 1), (13, 3), 'noise', (5, 5), False),
    'up10x': ((5, 7), (50, 70), 'steps', (5, 5), False),           # every window clipped at a border
    'white': ((40, 70), (29, 51), 'white', (7, 7), False),         # must stay 255 everywhere
}
MASK_CASES = ('kt9', 'ks17_4x')          # geometries of the masks
MASK_CHANNELS = (1, 3, 4)
MASK_VALUES = (0, 39, 40, 79, 80, 119, 120, 239, 240, 255)    # label boundaries of // 40 on both sides
INSIDE_WIDTHS = (1, 2, 3, 5, 61)

# ImagePreprocessor configurations: (final_dim, source (H, W), bot_pct_lim) -> (resize_dims (W, H), crop box)
PRE_CONFIGS = {
    'odd_planes': (((37, 61), (45, 77), (0.0, 0.0)), ((63, 37), (1, 0, 62, 37))),
    'narrow': (((23, 3), (30, 50), (0.0, 0.0)), ((38, 23), (17, 0, 20, 23))),
    'above': (((40, 63), (97, 151), (0.3, 0.5)), ((63, 40), (0, -16, 63, 24))),
}


def boxes(name):
    """[(label, (x0, y0, x1, y1))] in resized-image coordinates for case ``name``."""
    (_, (rh, rw), _, _, crops) = CASES[name]
    out = [('whole', (0, 0, rw, rh))]
    if not crops:
        return out
    for w in INSIDE_WIDTHS:                                   # odd origin, odd height; those that fit
        if 3 + w <= rw:
            out.append((f'inside{w}', (3, 1, 3 + w, min(rh, 12))))
    out.append(('overhang', (-5, -3, rw + 6, rh + 2)))        # all four sides at once
    out.append(('tiles_outside', (-70, -20, rw, rh)))         # first tile column and first tile row wholly outside
    out.append(('outside', (rw + 3, rh + 2, rw + 10, rh + 7)))   # nothing of the image: all 0 before the normalise
    return out


def image_runs():
    """Every (case, box label, box, flip) the fixture holds for images."""
    runs = []
    for name in CASES:
        for label, box in boxes(name):
            for flip in ((0, 1) if CASES[name][4] else (0,)):
                runs.append((name, label, box, flip))
    return runs


def out_key(name, label, flip):
    return f'{name}_{label}_f{flip}'


def mask_key(name, chans, flip=None):
    return f'mask_{name}_c{chans}' + ('' if flip is None else f'_f{flip}')


def load():
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, 'golden', 'image_edges.npz'))


def _span_cap(n_in, n_out, tile):
    scale = n_in / n_out
    support = 2.0 * max(scale, 1.0)
    return int(math.ceil((tile - 1) * scale + 2.0 * support)) + 2


def ksize(n_in, n_out):
    return int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def lds_bytes(src_hw, rs_hw, chans, nch):
    """launch() of csrc/preprocess.hip: rows_cap (pitch + 64 nch) + 4 (64 kx + 16 ky) bytes for a 16 x 64 tile, nch = 3
    (images) or 1 (masks) resampled channels of a ``chans``-channel source."""
    rows_cap = _span_cap(src_hw[0], rs_hw[0], 16)
    pitch = (_span_cap(src_hw[1], rs_hw[1], 64) * chans + 32 + 15) // 16 * 16
    return rows_cap * (pitch + 64 * nch) + 4 * (64 * ksize(src_hw[1], rs_hw[1]) + 16 * ksize(src_hw[0], rs_hw[0]))
