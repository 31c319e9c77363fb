"""Writes tests/golden/preprocess.npz: seeded uint8 frames and what Pillow makes of them through the reference dataset's
img_transform (dataset/nusc_mv_det_dataset.py:133-161: ``resize`` (bicubic), ``crop``, optional FLIP_LEFT_RIGHT) for the
evaluation-time crop of ``ida_resize_crop`` (dataset/...:433-446).  Pillow is the only image library used.

Per case ``<name>``: ``<name>_src`` u8 [H, W, C], ``<name>_out`` u8 [fH, fW, C] (``mask``: the labels
``(out / 40).astype(uint8)[..., 0]``, [fH, fW]), ``<name>_conf`` f64 [final H, final W, bot_pct_lim lo, hi, flip] and
``<name>_geom`` i64 [resized W, resized H, crop x0, y0, x1, y1].

    python tests/golden/make_golden_preprocess.py
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from sgv3d_amd.input_contract import ida_resize_crop  # noqa: E402  (numpy only)

# name: (source H, W, C), final_dim, bot_pct_lim, flip
CASES = {
    'dair': ((90, 160, 3), (72, 128), (0.0, 0.0), False),            # the DAIR ratio 0.8
    'odd_crop': ((97, 151, 3), (40, 64), (0.3, 0.5), False),         # odd downscale, crop box starts above the image
    'upscale': ((50, 70, 3), (77, 100), (0.0, 0.0), False),          # 1.54x upscale, horizontal crop
    'flip': ((135, 240, 3), (100, 176), (0.0, 0.1), True),           # flipped, off-centre crop
    'mask': ((90, 160, 3), (72, 128), (0.0, 0.0), True),             # 3-channel semantic mask, flipped
}


def pil_transform(src, resize_dims, box, flip):
    img = Image.fromarray(src).resize(resize_dims).crop(box)
    if flip:
        img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
    return np.array(img)


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    for name, ((h, w, c), final_dim, bot, flip) in CASES.items():
        if name == 'mask':   # label-like: blocks of a few values spread over 0..255
            src = np.repeat(np.repeat(rng.integers(0, 7, (h // 6 + 1, w // 8 + 1, c)) * 40 + 10, 6, 0), 8, 1)[:h, :w]
            src = src.astype(np.uint8)
        else:
            src = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        _, (rw, rh), box, _, _ = ida_resize_crop((h, w), final_dim, bot)
        res = pil_transform(src, (rw, rh), box, flip)
        if name == 'mask':
            res = (res / 40).astype(np.uint8)[..., 0]
        out[f'{name}_src'] = src
        out[f'{name}_out'] = res
        out[f'{name}_conf'] = np.array([final_dim[0], final_dim[1], bot[0], bot[1], float(flip)], np.float64)
        out[f'{name}_geom'] = np.array([rw, rh, *box], np.int64)
    np.savez_compressed(os.path.join(HERE, 'preprocess.npz'), **out)


if __name__ == '__main__':
    main()
