"""Writes tests/golden/image_edges.npz: tiny seeded uint8 frames and what Pillow makes of them at the geometries of
tests/image_edges.py -- every tap-count template of csrc/preprocess.hip, anisotropic resizes, the 4x downscale that needs
more than 64 KB of LDS, output widths that are no multiple of 4, and crop boxes that hang over each side of the resized
image or miss it.  Pillow is the only image library used: ``Image.fromarray(src).resize((rw, rh), Image.BICUBIC).crop(box)``
and optionally ``transpose(FLIP_LEFT_RIGHT)``, as the reference dataset's img_transform does
(dataset/nusc_mv_det_dataset.py:133-161); masks end as ``(out / 40).astype(uint8)[..., 0]`` (:603-614).

Images, per case ``<name>``: ``<name>_src`` u8 [H, W, 3], ``<name>_geom`` i64 [resized W, resized H], ``<name>_boxes``
i64 [n, 4] (x0, y0, x1, y1 in resized coordinates, in the order of ``image_edges.boxes``) and one
``<name>_<box label>_f<flip>`` u8 [box H, box W, 3] per box and flip.  Masks: ``mask_<name>_c<channels>`` u8 [H, W, C]
(``<name>``'s geometry, whole image) and ``mask_<name>_c<channels>_f<flip>`` u8 [rh, rw] labels.

The maker asserts what each case is there for: its pair of kernel sizes, accumulators beyond both ends of 0..255 in both
passes where the case is about clipping, and white staying white.

    python tests/golden/make_golden_image_edges.py
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_edges as E  # noqa: E402  (the case table)
import preprocess_ref as R  # noqa: E402  (numpy only; for the assertions, never for the outputs)

CLIPPING = {'ks13_steps': (1206, 249), 'aniso_a': None}   # accumulators below 0 = above 255: (horizontal, vertical) pass


def content(kind, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'steps':      # 0 / 255 blocks 5 wide and 7 tall
        return np.repeat((((xx // 5 + yy // 7) % 2) * 255).astype(np.uint8)[..., None], 3, 2)
    if kind == 'checker':    # 0 / 255 blocks 2 wide and 3 tall
        return np.repeat((((xx // 2 + yy // 3) % 2) * 255).astype(np.uint8)[..., None], 3, 2)
    return np.full((h, w, 3), 255, np.uint8)


def pil_transform(img, resize_dims, box, flip):
    img = img.resize(resize_dims, Image.BICUBIC).crop(box)
    if flip:
        img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
    return np.array(img)


def pil_image(src):
    """A PIL image of independent 8-bit bands: L, RGB, or CMYK for four (RGBA would be resized premultiplied by alpha)."""
    h, w, c = src.shape
    if c == 1:
        return Image.fromarray(src[..., 0])
    if c == 3:
        return Image.fromarray(src)
    return Image.frombytes('CMYK', (w, h), np.ascontiguousarray(src).tobytes())


def unclipped(img, axis, out_size):
    """The >> 22 accumulators of one pass of Pillow's resampler, before the clip to 0..255."""
    b, k = R.coeffs(img.shape[axis], out_size)
    src = img.astype(np.int64)
    shape = [1] * img.ndim
    shape[axis] = out_size
    acc = np.full(img.shape[:axis] + (out_size,) + img.shape[axis + 1:], 1 << (R.PRECISION_BITS - 1), np.int64)
    for t in range(k.shape[1]):
        acc += np.take(src, np.minimum(b[:, 0] + t, img.shape[axis] - 1), axis=axis) * k[:, t].reshape(shape)
    return acc >> R.PRECISION_BITS


def clip_counts(src, rw, rh):
    """((below 0, above 255) of the horizontal pass, the same of the vertical pass)."""
    a = unclipped(src, 1, rw)
    b = unclipped(np.clip(a, 0, 255).astype(np.uint8), 0, rh)
    return (int((a < 0).sum()), int((a > 255).sum())), (int((b < 0).sum()), int((b > 255).sum()))


def main():
    rng = np.random.default_rng(20261019)
    out = {}
    for name, ((h, w), (rh, rw), kind, ks, _) in E.CASES.items():
        assert (R.coeffs(w, rw)[1].shape[1], R.coeffs(h, rh)[1].shape[1]) == ks, name
        assert (E.ksize(w, rw), E.ksize(h, rh)) == ks, name
        src = content(kind, h, w, rng)
        out[f'{name}_src'] = src
        out[f'{name}_geom'] = np.array([rw, rh], np.int64)
        out[f'{name}_boxes'] = np.array([b for _, b in E.boxes(name)], np.int64)
        if name in CLIPPING:
            hc, vc = clip_counts(src, rw, rh)
            assert min(hc) >= 1 and min(vc) >= 1, (name, hc, vc)
            if CLIPPING[name]:
                assert (hc, vc) == ((CLIPPING[name][0],) * 2, (CLIPPING[name][1],) * 2), (name, hc, vc)
    for name, label, box, flip in E.image_runs():
        res = pil_transform(Image.fromarray(out[f'{name}_src']), tuple(out[f'{name}_geom']), box, flip)
        assert res.shape == (box[3] - box[1], box[2] - box[0], 3)
        if label == 'outside':
            assert not res.any()
        out[E.out_key(name, label, flip)] = res
    assert (out[E.out_key('white', 'whole', 0)] == 255).all() and (out[E.out_key('one_pixel', 'whole', 0)] == 255).all()

    for name in E.MASK_CASES:
        (h, w), (rh, rw) = E.CASES[name][:2]
        for c in E.MASK_CHANNELS:   # label-like: blocks 6 tall and 8 wide of values on both sides of the // 40 boundaries
            pick = rng.integers(0, len(E.MASK_VALUES), (h // 6 + 1, w // 8 + 1, c))
            src = np.repeat(np.repeat(np.asarray(E.MASK_VALUES, np.uint8)[pick], 6, 0), 8, 1)[:h, :w]
            assert all((src[..., 0] == v).any() for v in (39, 40, 79, 80, 239, 240))
            out[E.mask_key(name, c)] = src
            for flip in (0, 1):
                res = pil_transform(pil_image(src), (rw, rh), (0, 0, rw, rh), flip)
                res = res[..., None] if res.ndim == 2 else res
                out[E.mask_key(name, c, flip)] = (res / 40).astype(np.uint8)[..., 0]
    np.savez_compressed(os.path.join(HERE, 'image_edges.npz'), **out)


if __name__ == '__main__':
    main()
