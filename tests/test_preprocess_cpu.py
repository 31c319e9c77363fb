"""CPU: the Pillow resampler restated in numpy (tests/preprocess_ref.py) against the committed Pillow outputs and against
Pillow itself; the library's host-only coefficient tables against that restatement; the preprocessor's augmentation matrix;
argument checks that need no GPU."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
import preprocess_ref as R

CASES = ('dair', 'odd_crop', 'upscale', 'flip', 'mask')


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "preprocess.npz"))


def _case(d, name):
    conf, geom = d[f'{name}_conf'], d[f'{name}_geom']
    final_dim = (int(conf[0]), int(conf[1]))
    return d[f'{name}_src'], d[f'{name}_out'], final_dim, (float(conf[2]), float(conf[3])), bool(conf[4]), \
        (int(geom[0]), int(geom[1])), tuple(int(v) for v in geom[2:])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(fixture, name):
    from sgv3d_amd.input_contract import ida_resize_crop
    src, want, final_dim, bot, flip, dims, box = _case(fixture, name)
    _, dims2, box2, _, _ = ida_resize_crop(src.shape[:2], final_dim, bot)
    assert (tuple(dims2), tuple(box2)) == (dims, box)
    got = R.transform(src, dims, box, flip)
    if name == 'mask':
        got = R.mask_labels(got)
    assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("src_hw,size", [((90, 160), (128, 72)), ((135, 240), (192, 108)), ((108, 192), (153, 86)),
                                         ((50, 70), (33, 77)), ((64, 64), (100, 17)), ((37, 53), (53, 37)),
                                         ((200, 301), (76, 50)), ((40, 40), (40, 40)), ((33, 97), (97, 33))])
def test_restatement_matches_pillow(src_hw, size):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(src_hw[0] * 1000 + size[0])
    for shape in (src_hw + (3,), src_hw):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(R.resize(img, size), np.array(Image.fromarray(img).resize(size)))


@pytest.mark.parametrize("n_in,n_out", [(1920, 1536), (1080, 864), (160, 128), (151, 64), (70, 107), (64, 17),
                                        (240, 177), (10, 10), (400, 100), (5, 300)])
def test_library_coefficients_equal_restatement(n_in, n_out):
    from sgv3d_amd.preprocess import resample_coeffs
    b, k = resample_coeffs(n_in, n_out)
    b2, k2 = R.coeffs(n_in, n_out)
    assert b.dtype == np.int32 and k.dtype == np.int32
    assert np.array_equal(b, b2) and np.array_equal(k, k2)


def test_coefficients_reject_bad_sizes():
    from sgv3d_amd import _lib
    lib = _lib.load()
    ks = ctypes.c_int(-7)
    for a, b in ((0, 10), (10, 0), (-3, 4)):
        assert lib.sgv3d_resample_coeffs(a, b, None, None, ctypes.byref(ks)) == -1
        assert b"non-positive" in lib.sgv3d_last_error()
    assert lib.sgv3d_resample_coeffs(401, 100, None, None, ctypes.byref(ks)) == -1      # 4.01x
    assert b"above 4x" in lib.sgv3d_last_error()
    assert lib.sgv3d_resample_coeffs(400, 100, None, None, ctypes.byref(ks)) == 0 and ks.value == 17
    from sgv3d_amd.preprocess import resample_coeffs
    from sgv3d_amd._lib import SGV3DError
    with pytest.raises(SGV3DError, match="above 4x"):
        resample_coeffs(1080, 200)


def test_launch_arguments_rejected_without_gpu():
    """Bad launch arguments fail before any HIP call (null pointers stand in for device buffers)."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    m = (ctypes.c_float * 3)(1, 2, 3)
    s = (ctypes.c_float * 3)(1, 1, 1)
    rc = lib.sgv3d_preprocess_images(0, 1080, 1920, 864, 1536, 0, 0, 864, 1536, 0, 1, None, None, 7, None, None, 7, m, s,
                                     None, None, None)
    assert rc == -1 and b"non-positive" in lib.sgv3d_last_error()
    rc = lib.sgv3d_preprocess_images(1, 1080, 1920, 200, 1536, 0, 0, 200, 1536, 0, 1, None, None, 7, None, None, 7, m, s,
                                     None, None, None)
    assert rc == -1 and b"above 4x" in lib.sgv3d_last_error()
    rc = lib.sgv3d_preprocess_images(1, 1080, 1920, 864, 1536, 0, 0, 864, 1536, 0, 1, None, None, 5, None, None, 7, m, s,
                                     None, None, None)
    assert rc == -1 and b"coefficient tables" in lib.sgv3d_last_error()
    rc = lib.sgv3d_preprocess_images(1, 1080, 1920, 864, 1536, 0, 0, 864, 1536, 0, 1, None, None, 7, None, None, 7, m, s,
                                     None, None, None)
    assert rc == -1 and b"null pointer" in lib.sgv3d_last_error()
    rc = lib.sgv3d_preprocess_mask(1, 90, 160, 0, 72, 128, 0, 0, 72, 128, 0, None, None, 7, None, None, 7, None, None,
                                   None)
    assert rc == -1 and b"non-positive" in lib.sgv3d_last_error()


@pytest.mark.parametrize("flip", [False, True])
def test_preprocessor_ida_matrix(flip):
    from sgv3d_amd.input_contract import ida_matrix, ida_resize_crop
    from sgv3d_amd.preprocess import ImagePreprocessor
    conf = {'final_dim': (40, 64), 'bot_pct_lim': (0.3, 0.5)}
    img_conf = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)
    pre = ImagePreprocessor(conf, img_conf, src_hw=(97, 151), flip=flip, device='cpu')
    resize, dims, crop, _, _ = ida_resize_crop((97, 151), (40, 64), (0.3, 0.5))
    assert pre.resize_dims == tuple(dims) and pre.crop == tuple(crop)
    assert np.array_equal(pre.ida, ida_matrix(resize, crop, flip, 0.0))
    assert pre.ida.dtype == np.float32
    with pytest.raises(NotImplementedError):
        ImagePreprocessor(conf, img_conf, src_hw=(97, 151), rotate=5.0, device='cpu')


def test_normalize_restatement():
    """mmcv.imnormalize's arithmetic: float32 subtraction, then a float32 multiply by f32(1 / f64(std)); R<->B swap first."""
    img = np.arange(6 * 3, dtype=np.uint8).reshape(2, 3, 3) * 13
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    out = R.normalize(img, mean, std, True)
    assert out.shape == (3, 2, 3) and out.dtype == np.float32
    for c in range(3):
        x = img[..., 2 - c].astype(np.float32)
        want = (x - np.float32(mean[c])) * np.float32(1.0 / np.float64(np.float32(std[c])))
        assert np.array_equal(out[c], want)
