"""CPU: the training-time augmentation restated in numpy (tests/train_augment_ref.py) against the reference's own outputs
(tests/golden/train_augment.npz) and against Pillow; the library's host coefficient tables; the seeded draws, the
rectified matrices and transform_pitch; the brightness rules; argument checks that need no GPU.

The brightness restatement (cv2.cvtColor BGR2GRAY's 14-bit weights, convertScaleAbs's rounding) is pinned only by the
rules written down here: OpenCV is not available to compare against."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
import preprocess_ref as P
import train_augment_ref as R

CASES = ('down', 'up', 'one_axis', 'large_kernel', 'unit', 'pitch_off', 'mask')
CONF = dict(final_dim=(72, 128), bot_pct_lim=(0.0, 0.0))
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "train_augment.npz"))


@pytest.mark.parametrize("skip_unchanged", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(fixture, name, skip_unchanged):
    """Every case byte for byte; running the resize pass of an unchanged axis (identity coefficients) changes nothing."""
    ratio, roll, tp = fixture[f'{name}_args']
    got = R.intrin_extrin_transform(fixture[f'{name}_src'], ratio, roll, int(tp), fixture[f'{name}_intrin'],
                                    skip_unchanged)
    assert np.array_equal(got, fixture[f'{name}_out'])


@pytest.mark.parametrize("src_hw,size", [((90, 160), (133, 75)), ((90, 160), (161, 90)), ((135, 240), (72, 40)),
                                         ((50, 70), (90, 111)), ((64, 64), (7, 3)), ((40, 40), (40, 40))])
def test_lanczos_restatement_matches_pillow(src_hw, size):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(src_hw[0] * 1000 + size[0])
    for shape in (src_hw + (3,), src_hw):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(R.resize(img, size), np.array(Image.fromarray(img).resize(size, Image.LANCZOS)))


def test_rotate_matrix_is_pillows():
    from sgv3d_amd.train_augment import rotate_matrix
    for angle, center, tr in ((1.3, (80, 44), (0, 2)), (-2.7, (951, 541), (0, -38)), (0.0, (5, 7), (0, 0)),
                              (-0.004, (960, 540), (0, 61))):
        assert rotate_matrix(angle, center, tr) == R.rotate_matrix(angle, center, tr)


@pytest.mark.parametrize("n_in,n_out", [(1920, 1536), (1080, 864), (1920, 2304), (1920, 500), (1080, 200), (160, 161),
                                        (240, 72), (5, 300), (1080, 1080), (1920, 1)])
def test_library_coefficients_equal_restatement(n_in, n_out):
    from sgv3d_amd.preprocess import resample_coeffs
    from sgv3d_amd.train_augment import FILTER_BICUBIC, FILTER_LANCZOS, resample_coeffs_filter
    for filt, name in ((FILTER_BICUBIC, 'bicubic'), (FILTER_LANCZOS, 'lanczos')):
        b, k = resample_coeffs_filter(filt, n_in, n_out)
        b2, k2 = R.coeffs(n_in, n_out, name)
        assert b.dtype == np.int32 and k.dtype == np.int32
        assert np.array_equal(b, b2) and np.array_equal(k, k2), name
    if n_in <= 4 * n_out:                      # the eval-time symbol is unchanged and agrees
        b, k = resample_coeffs(n_in, n_out)
        b2, k2 = resample_coeffs_filter(FILTER_BICUBIC, n_in, n_out)
        assert np.array_equal(b, b2) and np.array_equal(k, k2)


def test_identity_coefficients_are_exact():
    b, k = R.coeffs(1920, 1920, 'lanczos')
    assert np.array_equal(b[:, 1] > 0, np.ones(1920, bool))
    for o in range(1920):
        taps = k[o, :b[o, 1]]
        assert taps[o - b[o, 0]] == 1 << R.PRECISION_BITS and np.count_nonzero(taps) == 1


def test_sample_params_reproduce_the_seeded_draws(fixture):
    from sgv3d_amd.train_augment import sample_params
    seed = int(fixture['draw_seed'])
    p = sample_params(len(fixture['draw_ie']), random.Random(seed), np.random.RandomState(seed))
    ie, bright = fixture['draw_ie'], fixture['draw_bright']
    assert np.array_equal(p.ie, ie) and np.array_equal(p.bright, bright)
    assert np.array_equal(p.ratio[ie], fixture['draw_ratio'][ie])
    assert np.array_equal(p.roll_deg[ie], fixture['draw_roll'][ie])
    assert np.array_equal(p.u[bright], fixture['draw_u'][bright])


def test_rectify_and_augment_camera_match_the_reference(fixture):
    from sgv3d_amd.input_contract import collate_mats
    from sgv3d_amd.train_augment import augment_camera, rectify, sample_params
    seed = int(fixture['draw_seed'])
    n = len(fixture['draw_ie'])
    p = sample_params(n, random.Random(seed), np.random.RandomState(seed))
    K, e2s = fixture['cam_intrin'], fixture['cam_e2s']
    cam = dict(sensor2ego=np.linalg.inv(e2s.astype(np.float64)), intrin=K, ida=np.eye(4), bda=np.eye(4))
    cams = []
    for i in range(n):
        if p.ie[i]:
            Kr, Er, tp = rectify(K, e2s, p.ratio[i], p.roll_deg[i], p.pitch_deg[i])
            assert np.array_equal(Kr, fixture['draw_intrin'][i]) and np.array_equal(Er, fixture['draw_e2s'][i])
            assert tp == fixture['draw_tp'][i]
        c = augment_camera(cam, p, i)
        assert p.transform_pitch[i] == c['transform_pitch'] == fixture['draw_tp'][i]
        assert tuple(p.center[i]) == c['center'] == (int(K[0, 2]), int(K[1, 2]))
        np.testing.assert_allclose(c['intrin'], fixture['draw_intrin'][i], rtol=1e-6)
        np.testing.assert_allclose(np.linalg.inv(c['sensor2ego']), fixture['draw_e2s'][i], rtol=1e-5, atol=1e-5)
        s2s = c['sensor2sensor']
        np.testing.assert_allclose(np.linalg.inv(s2s), e2s @ np.linalg.inv(fixture['draw_e2s'][i]), rtol=1e-5,
                                   atol=1e-5)
        cams.append(c)
    mats = collate_mats(cams)
    assert mats['intrin_mats'].shape == (n, 1, 1, 4, 4)
    s2v = mats['sensor2virtual_mats'].view(n, 16).numpy()
    changed = np.abs(s2v - s2v[~p.ie][0]).max(1) > 1e-4
    assert np.array_equal(changed, p.ie)                         # the rectified pose tilts the ground plane


def test_gray_and_brightness_rules():
    img = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
    # channel 0 carries B's weight: (c0 1868 + c1 9617 + c2 4899 + 8192) >> 14
    assert R.gray_sum(img[:, :1]) == (255 * 1868 + 8192) >> 14 == 29
    assert R.gray_sum(img[:, 2:3]) == (255 * 4899 + 8192) >> 14 == 76
    assert R.gray_sum(img) == 29 + 150 + 76 + ((10 * 1868 + 20 * 9617 + 30 * 4899 + 8192) >> 14)
    assert R.beta_of(0, 1, 0.9) == 50 and R.beta_of(0, 1, 0.3) == pytest.approx(30.0)
    assert R.beta_of(255 * 4, 4, 0.5) == -50 and R.beta_of(120 * 2, 2, 0.5) == pytest.approx(-10.0)
    assert R.beta_of(100, 1, 0.7) == 0                           # beta == 0 takes the negative branch: -0.0
    ties = np.array([[[10, 11, 12]]], np.uint8)
    assert R.scale_abs(ties, 0.5).tolist() == [[[10, 12, 12]]]   # 10.5 -> 10, 11.5 -> 12, 12.5 -> 12
    assert R.scale_abs(ties, -12.5).tolist() == [[[2, 2, 0]]]    # |x + beta|: -2.5 -> 2, -1.5 -> 2, -0.5 -> 0
    assert R.scale_abs(np.array([[[250]]], np.uint8), 49.0).tolist() == [[[255]]]


def _params(**kw):
    from sgv3d_amd.train_augment import AugmentParams
    n = len(kw['ie'])
    d = dict(ratio=[1.0] * n, roll_deg=[0.0] * n, pitch_deg=[0.0] * n, bright=[False] * n, u=[0.0] * n,
             center=[(80, 45)] * n, transform_pitch=[0] * n)
    d.update(kw)
    return AugmentParams(**d)


def test_plan_rejects_bad_parameters_without_gpu():
    from sgv3d_amd.train_augment import AugmentParams, TrainAugmenter
    aug = TrainAugmenter(CONF, IMG_CONF, src_hw=(90, 160), device='cpu')
    rec, tables, n = aug.plan(_params(ie=[True, False, True], ratio=[0.9, 1.0, 1.3]), 3)
    assert n == 2 and rec['slot'][2] == 1 and rec['rs_w'][0] == 144 and rec['off_x'][2] == 24
    assert rec['xtab'][2] + rec['rs_w'][2] * (2 + rec['kx'][2]) <= tables.size
    with pytest.raises(ValueError, match="> 0"):
        aug.plan(_params(ie=[True], ratio=[0.01]), 1)             # 90 x 0.01 -> 0 rows
    with pytest.raises(ValueError, match="parameter sets"):
        aug.plan(_params(ie=[True]), 2)
    unplaced = AugmentParams([True], [0.9], [1.0], [0.1], [False], [0.0])
    with pytest.raises(ValueError, match="augment_camera"):
        aug.plan(unplaced, 1)
    # a very small ratio is fine while the size stays >= 1 pixel (a 21-tap kernel at 0.3)
    rec, _, _ = aug.plan(_params(ie=[True], ratio=[0.3]), 1)
    assert rec['kx'][0] == 21 and rec['ky'][0] == 21


def test_abi_rejects_bad_arguments_without_gpu():
    from sgv3d_amd import _lib
    from sgv3d_amd.train_augment import FRAME_DTYPE
    lib = _lib.load()
    assert FRAME_DTYPE.itemsize == 112
    H, W, fH, fW = 90, 160, 72, 128
    xk = P.coeffs(W, 128)[1].shape[1]
    yk = P.coeffs(H, 72)[1].shape[1]
    mean = (ctypes.c_float * 3)(0, 0, 0)
    std = (ctypes.c_float * 3)(1, 1, 1)
    rec = np.zeros(1, FRAME_DTYPE)
    fake = 4096                                              # device pointers are never touched by the checks
    need = lib.sgv3d_augment_workspace_bytes(1, 1, H, W, fH, fW, 0)
    assert need >= 2 * H * W * 3 + fH * fW * 3 + 8

    def call(frames=1, rec=rec, work_bytes=need, xksize=xk, tables_len=1 << 20):
        return lib.sgv3d_augment_images(frames, H, W, rec.ctypes.data, fake, fake, tables_len, 72, 128, 0, 0, fH, fW,
                                        1, fake, fake, xksize, fake, fake, yk, mean, std, fake, fake, work_bytes, fake,
                                        None)
    assert call(frames=0) == -1 and b"non-positive" in lib.sgv3d_last_error()
    assert call(xksize=xk + 2) == -1 and b"coefficient" in lib.sgv3d_last_error()
    bad = rec.copy()
    bad['ie'] = 1                                            # rectified with a 0 x 0 resize
    assert call(rec=bad) == -1 and b"below one pixel" in lib.sgv3d_last_error()
    bad['rs_w'], bad['rs_h'], bad['kx'], bad['ky'] = 144, 81, 9, 9
    assert call(rec=bad, tables_len=10) == -1 and b"out of range" in lib.sgv3d_last_error()
    bad['affine'][0] = np.nan
    assert call(rec=bad) == -1 and b"affine" in lib.sgv3d_last_error()
    bad = rec.copy()
    bad['bright'] = 2
    assert call(rec=bad) == -1
    assert call(work_bytes=16) == -3 and b"workspace" in lib.sgv3d_last_error()
    m = rec.copy()
    m['bright'] = 1
    assert lib.sgv3d_augment_mask(1, H, W, 3, m.ctypes.data, fake, fake, 0, 72, 128, 0, 0, fH, fW, fake, fake, xk,
                                  fake, fake, yk, fake, fake, 1 << 30, fake, None) == -1
    assert lib.sgv3d_resample_coeffs_filter(7, 10, 10, None, None, None) == -1
    assert lib.sgv3d_augment_workspace_bytes(0, 0, H, W, fH, fW, 0) == 0
