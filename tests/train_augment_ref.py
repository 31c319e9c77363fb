"""Numpy restatement of the reference dataset's training-time camera augmentation (test helper, no library calls):
``img_intrin_extrin_transform`` (dataset/nusc_mv_det_dataset.py:94-110: Pillow LANCZOS resize, paste into a black canvas or
crop, ``Image.rotate`` with BICUBIC resampling about the intrinsic centre plus a vertical translate) and the brightness
jitter of :618-623 (``cv2.cvtColor(img, COLOR_BGR2GRAY)`` mean, ``cv2.convertScaleAbs(img, 1.0, beta)``).

Pillow parts restated from its src/libImaging: Resample.c (precompute_coeffs with ``lanczos_filter``, the 8-bit integer
passes) and Geometry.c (ImagingGenericTransform with ``affine_transform`` and ``bicubic_filter32RGB``), settled against
tests/golden/train_augment.npz.  The OpenCV parts are restated from its documented 8-bit rules (the 14-bit fixed-point
gray weights, ``saturate_cast`` rounding to nearest even); OpenCV itself is not available to pin them against."""
import math

import numpy as np

import preprocess_ref as P

PRECISION_BITS = P.PRECISION_BITS


def lanczos(x):
    """Pillow's lanczos_filter: sinc(x) sinc(x / 3) on [-3, 3)."""
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    if -3.0 <= x < 3.0:
        return sinc(x) * sinc(x / 3)
    return 0.0


FILTERS = {'bicubic': (P.bicubic, 2.0), 'lanczos': (lanczos, 3.0)}


def coeffs(in_size, out_size, filt='lanczos'):
    """(bounds int32 [out, 2] = first input pixel and tap count, coeffs int32 [out, ksize]) of Pillow's precompute_coeffs +
    normalize_coeffs_8bpc for ``filt``."""
    f, support0 = FILTERS[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = support0 * fs
    ss = 1.0 / fs
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ks), np.int32)
    for o in range(out_size):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        k[o, :n] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        bounds[o] = (xmin, n)
    return bounds, k


def _pass(img, axis, out_size, filt):
    in_size = img.shape[axis]
    b, k = coeffs(in_size, out_size, filt)
    src = img.astype(np.int64)
    shape = [1] * img.ndim
    shape[axis] = out_size
    acc = np.full(img.shape[:axis] + (out_size,) + img.shape[axis + 1:], 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(k.shape[1]):
        idx = np.minimum(b[:, 0] + t, in_size - 1)          # (past a window's taps the weight is 0)
        acc += np.take(src, idx, axis=axis) * k[:, t].reshape(shape)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, size, filt='lanczos', skip_unchanged=True):
    """PIL ``Image.resize(size, filt)`` of a uint8 [H, W] or [H, W, C] array; size = (W, H).  Pillow skips the pass of an
    axis whose size does not change; ``skip_unchanged=False`` runs it anyway (identity coefficients)."""
    w, h = size
    if w < 1 or h < 1:
        raise ValueError("height and width must be > 0")
    out = img
    if w != img.shape[1] or not skip_unchanged:
        out = _pass(out, 1, w, filt)
    if h != img.shape[0] or not skip_unchanged:
        out = _pass(out, 0, h, filt)
    return out


def scale_offsets(h, w, ratio, center):
    """(resized (W, H), (off_x, off_y)): canvas pixel (y, x) = resized pixel (y + off_y, x + off_x), 0 outside it
    (dataset/...:98-108)."""
    new_w, new_h = int(w * ratio), int(h * ratio)
    h_min = int(center[1] * abs(1.0 - ratio))
    w_min = int(center[0] * abs(1.0 - ratio))
    sgn = -1 if ratio <= 1.0 else 1
    return (new_w, new_h), (sgn * w_min, sgn * h_min)


def place(img, h, w, off):
    """Paste / crop of ``img`` into an h x w black canvas: out[y, x] = img[y + off_y, x + off_x] where that exists."""
    ox, oy = off
    out = np.zeros((h, w) + img.shape[2:], np.uint8)
    y0, y1 = max(0, -oy), min(h, img.shape[0] - oy)
    x0, x1 = max(0, -ox), min(w, img.shape[1] - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = img[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def rotate_matrix(angle, center, translate):
    """The six inverse-affine coefficients ``Image.rotate(angle, center=center, translate=translate)`` passes on."""
    angle = angle % 360.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -center[0] - translate[0], -center[1] - translate[1]
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += center[0]
    m[5] += center[1]
    return m


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine_bicubic(img, m):
    """ImagingGenericTransform(affine, bicubic) of a uint8 [H, W] or [H, W, C] image into the same size, fill 0."""
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xin = m[0] * (xx + 0.5) + m[1] * (yy + 0.5) + m[2]
    yin = m[3] * (xx + 0.5) + m[4] * (yy + 0.5) + m[5]
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xs, ys = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x, y = np.floor(xs), np.floor(ys)
    dx, dy = xs - x, ys - y
    x, y = x.astype(np.int64) - 1, y.astype(np.int64) - 1
    src = img.astype(np.float64)
    if src.ndim == 2:
        src = src[..., None]
    cols = [np.clip(x + i, 0, w - 1) for i in range(4)]
    rows = []
    for j in range(4):
        r = np.clip(y + j, 0, h - 1)
        rows.append(_cubic(*(src[r, c] for c in cols), dx[..., None]))
    v = _cubic(*rows, dy[..., None])
    out = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, v)).astype(np.uint8)   # (v in (0, 255): truncation)
    out = np.where(inside[..., None], out, 0).astype(np.uint8)
    return out if img.ndim == 3 else out[..., 0]


def intrin_extrin_transform(img, ratio, roll, transform_pitch, intrin, skip_unchanged=True):
    """img_intrin_extrin_transform (dataset/...:94-110) of a uint8 [H, W, C] (or [H, W]) array."""
    c = np.asarray(intrin)[:2, 2].astype(np.int32)
    center = (int(c[0]), int(c[1]))
    h, w = img.shape[:2]
    size, off = scale_offsets(h, w, ratio, center)
    canvas = place(resize(img, size, 'lanczos', skip_unchanged), h, w, off)
    return affine_bicubic(canvas, rotate_matrix(-roll, center, (0, transform_pitch)))


def gray_sum(img):
    """Sum of cv2.cvtColor(img, COLOR_BGR2GRAY) over an RGB-ordered uint8 [H, W, 3] image (channel 0 weighted as B)."""
    x = img.astype(np.int64)
    g = (x[..., 0] * 1868 + x[..., 1] * 9617 + x[..., 2] * 4899 + 8192) >> 14
    return int(g.sum())


def beta_of(gsum, npix, u):
    """dataset/...:620-622: beta = u (100 - mean gray), magnitude clamped to 50."""
    mean = gsum / npix
    beta = u * (100 - mean)
    return (1 if beta > 0 else -1) * min(abs(beta), 50)


def scale_abs(img, beta):
    """cv2.convertScaleAbs(img, alpha=1.0, beta=beta) on uint8: saturate_cast<uchar>(|x * 1.0f + (float)beta|)."""
    v = np.abs(img.astype(np.float32) * np.float32(1.0) + np.float32(beta))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def brightness(img, u):
    return scale_abs(img, beta_of(gray_sum(img), img.shape[0] * img.shape[1], u))
