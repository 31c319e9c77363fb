"""Numpy restatement of the reference dataset's image path (test helper, no library calls): Pillow's 8-bit bicubic resize
(src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / _Vertical_8bpc),
PIL's crop and left-right flip (dataset/nusc_mv_det_dataset.py:133-161 img_transform), mmcv.imnormalize (:624) and the
semantic-mask rule (:603-614)."""
import math

import numpy as np

PRECISION_BITS = 22


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def coeffs(in_size, out_size):
    """(bounds int32 [out, 2] = first input pixel and tap count, coeffs int32 [out, ksize])."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ks), np.int32)
    for o in range(out_size):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        k[o, :n] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        bounds[o] = (xmin, n)
    return bounds, k


def _pass(img, axis, out_size):
    """One separable pass along ``axis`` of a uint8 array."""
    in_size = img.shape[axis]
    b, k = coeffs(in_size, out_size)
    src = img.astype(np.int32)
    shape = [1] * img.ndim
    shape[axis] = out_size
    acc = np.full(img.shape[:axis] + (out_size,) + img.shape[axis + 1:], 1 << (PRECISION_BITS - 1), np.int32)
    for t in range(k.shape[1]):
        idx = np.minimum(b[:, 0] + t, in_size - 1)          # (past a window's taps the weight is 0)
        acc += np.take(src, idx, axis=axis) * k[:, t].reshape(shape)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, size):
    """PIL ``Image.resize(size)`` (bicubic) of a uint8 [H, W] or [H, W, C] array; size = (W, H) as PIL takes it."""
    w, h = size
    out = img
    if w != img.shape[1]:
        out = _pass(out, 1, w)
    if h != img.shape[0]:
        out = _pass(out, 0, h)
    return out


def crop(img, box):
    """PIL ``crop(box)``: (left, upper, right, lower); pixels outside the image are 0."""
    x0, y0, x1, y1 = box
    out = np.zeros((y1 - y0, x1 - x0) + img.shape[2:], img.dtype)
    sx0, sy0 = max(x0, 0), max(y0, 0)
    sx1, sy1 = min(x1, img.shape[1]), min(y1, img.shape[0])
    if sx0 < sx1 and sy0 < sy1:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = img[sy0:sy1, sx0:sx1]
    return out


def transform(img, resize_dims, box, flip):
    """img_transform's pixel part for rotate = 0: resize, crop, optional left-right flip."""
    out = crop(resize(img, resize_dims), box)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def normalize(img, mean, std, to_rgb):
    """mmcv.imnormalize(img, mean, std, to_rgb) + HWC -> CHW: float32 (x - mean) * f32(1 / f64(std))."""
    x = img.astype(np.float32)
    if to_rgb:
        x = x[..., ::-1]
    mean = np.asarray(mean, np.float32).reshape(1, 1, 3)
    stdinv = (1.0 / np.asarray(std, np.float32).astype(np.float64)).astype(np.float32).reshape(1, 1, 3)
    return np.ascontiguousarray(((x - mean) * stdinv).transpose(2, 0, 1))


def mask_labels(transformed_mask):
    """(np.array(mask) / 40).astype(uint8)[..., 0] of an already transformed HWC mask."""
    return (transformed_mask / 40).astype(np.uint8)[..., 0]
