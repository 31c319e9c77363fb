"""GPU: csrc/preprocess.hip and stages C / D of csrc/augment.hip at every kernel form and edge geometry, bit for bit
against Pillow's bytes (tests/golden/image_edges.npz) and the numpy restatements (tests/preprocess_ref.py,
tests/train_augment_ref.py).  Reads fixtures only.

preprocess.hip is called through the C ABI (only it takes anisotropic resizes and crop boxes left of the image): every
tap-count template (ksize 5, 7, 9, 13, 17, and kx != ky), the tiles above 64 KB of LDS, output widths 1, 2, 3, 5, 61 and
other non-multiples of 4 (the scalar store tails of images and masks), crop boxes hanging over each side and missing the
image, with and without the flip, three frames per launch at unaligned bases, sources at every byte alignment, masks of
1, 3 and 4 channels.  Every destination lies between guard bands inside a pre-filled buffer."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import image_edges as E
import preprocess_ref as P
import train_augment_ref as R
from test_train_augment_gpu import IMG_CONF, UNIT_CONF, _placed, _restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256
RUNS = E.image_runs()
FX = None


def _fx():
    global FX
    if FX is None:
        FX = E.load()
    return FX


@functools.lru_cache(maxsize=None)
def _tables(n_in, n_out):
    from sgv3d_amd.preprocess import resample_coeffs
    b, k = resample_coeffs(n_in, n_out)
    return torch.from_numpy(b).to(DEV), torch.from_numpy(k).to(DEV), k.shape[1]


def _three(src):
    """The frames of one call: the source, reversed top to bottom, reversed left to right."""
    return np.ascontiguousarray(np.stack([src, src[::-1], src[:, ::-1]]))


@functools.lru_cache(maxsize=None)
def _resized(key, frame, rw, rh):
    """The restatement's resize of frame ``frame`` of fixture array ``key`` (computed once per session, read-only)."""
    out = P.resize(_three(_fx()[key])[frame], (rw, rh))
    out.setflags(write=False)
    return out


def _expected(key, frame, rs, box, flip):
    out = P.crop(_resized(key, frame, *rs), box)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def _launch(src_ptr, n, src_shape, rs, box, flip, swap_rb, mask, fill):
    """One sgv3d_preprocess_images / _mask call into a guarded buffer -> the destination region (numpy).  ``fill``: what
    the region holds before the launch."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    H, W, C = src_shape
    rw, rh = rs
    ow, oh = box[2] - box[0], box[3] - box[1]
    xb, xk, kx = _tables(W, rw)
    yb, yk, ky = _tables(H, rh)
    count = n * oh * ow * (1 if mask else 3)
    if mask:
        buf = torch.full((BAND + count + BAND,), fill, dtype=torch.uint8, device=DEV)
        buf[:BAND] = 0xA5
        buf[BAND + count:] = 0xA5
        guard = 0xA5
    else:
        buf = torch.full((BAND + count + BAND,), fill, dtype=torch.float32, device=DEV)
        buf[:BAND] = 12345.0
        buf[BAND + count:] = 12345.0
        guard = 12345.0
    dst = buf.data_ptr() + BAND * buf.element_size()
    geo = (rh, rw, box[0], box[1], oh, ow, int(flip))
    tabs = (xb.data_ptr(), xk.data_ptr(), kx, yb.data_ptr(), yk.data_ptr(), ky)
    stream = _lib.stream_handle(torch.device(DEV))
    if mask:
        rc = lib.sgv3d_preprocess_mask(n, H, W, C, *geo, *tabs, src_ptr, dst, stream)
    else:
        mean = (ctypes.c_float * 3)(*IMG_CONF['img_mean'])
        std = (ctypes.c_float * 3)(*IMG_CONF['img_std'])
        rc = lib.sgv3d_preprocess_images(n, H, W, *geo, int(swap_rb), *tabs, mean, std, src_ptr, dst, stream)
    _lib.check(rc, "preprocess")
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:BAND] == guard).all() and (raw[BAND + count:] == guard).all(), "a guard band was written"
    return raw[BAND:BAND + count].reshape((n, oh, ow) if mask else (n, 3, oh, ow))


def _run_images(frames, rs, box, flip, swap_rb, offset=None):
    """frames u8 [n, H, W, 3] through sgv3d_preprocess_images, twice -> float32 [n, 3, oh, ow].  ``offset``: start the
    frames that many bytes into a buffer with 64 bytes of 0xFF on both sides (None: a plain tensor)."""
    n = frames.shape[0]
    if offset is None:
        dev = torch.from_numpy(frames).to(DEV)
        ptr = dev.data_ptr()
    else:
        dev = torch.full((64 + 16 + frames.size + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        assert dev.data_ptr() % 16 == 0
        dev[64 + offset:64 + offset + frames.size] = torch.from_numpy(frames.reshape(-1)).to(DEV)
        ptr = dev.data_ptr() + 64 + offset
    got = _launch(ptr, n, frames.shape[1:], rs, box, flip, swap_rb, False, float('nan'))
    assert not np.isnan(got).any(), "an output value was never written"
    again = _launch(ptr, n, frames.shape[1:], rs, box, flip, swap_rb, False, float('nan'))
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "a repeat launch differs"
    return got


def _run_mask(frames, rs, box, flip):
    """frames u8 [n, H, W, C] through sgv3d_preprocess_mask into a 0xA5 and then a 0x5A pre-fill -> uint8 [n, oh, ow]."""
    dev = torch.from_numpy(frames).to(DEV)
    got = _launch(dev.data_ptr(), frames.shape[0], frames.shape[1:], rs, box, flip, 0, True, 0xA5)
    again = _launch(dev.data_ptr(), frames.shape[0], frames.shape[1:], rs, box, flip, 0, True, 0x5A)
    assert np.array_equal(got, again), "a label was never written, or a repeat launch differs"
    return got


def _norm(img, swap_rb):
    return P.normalize(img, IMG_CONF['img_mean'], IMG_CONF['img_std'], bool(swap_rb))


def _check_images(name, label, box, flip, swap_rb, offset=None):
    fx = _fx()
    key = f'{name}_src'
    rs = tuple(int(v) for v in fx[f'{name}_geom'])
    got = _run_images(_three(fx[key]), rs, box, flip, swap_rb, offset)
    want0 = fx[E.out_key(name, label, flip)]                       # Pillow's bytes
    assert np.array_equal(got[0], _norm(want0, swap_rb)), f"frame 0: {(got[0] != _norm(want0, swap_rb)).sum()} differ"
    for f in (1, 2):
        want = _norm(_expected(key, f, rs, box, flip), swap_rb)
        assert np.array_equal(got[f], want), f"frame {f}: {(got[f] != want).sum()} values differ"
    return got


@pytest.mark.parametrize("name,label,box,flip", RUNS, ids=[E.out_key(n, l, f) for n, l, _, f in RUNS])
def test_images_every_case_box_and_flip(name, label, box, flip):
    got = _check_images(name, label, box, flip, 1)
    if label == 'outside':      # nothing of the image: the normalised zero, everywhere
        zero = _norm(np.zeros(got.shape[2:] + (3,), np.uint8), 1)
        assert all(np.array_equal(g, zero) for g in got)


@pytest.mark.parametrize("name", ['kt9', 'ks17_4x'])
def test_images_without_channel_swap(name):
    for label, box in E.boxes(name):
        _check_images(name, label, box, 0, 0)


def test_exact_4x_downscale_takes_the_large_lds_tile():
    """64x132 -> 16x33 is the only kind of call that raises the kernel's dynamic LDS limit.  From launch():
    rows_cap = span_cap(64, 16, 16) = ceil(15 * 4 + 2 * 8) + 2 = 78 staged rows;
    pitch = roundup16(span_cap(132, 33, 64) * 3 + 32) = roundup16((ceil(63 * 4 + 16) + 2) * 3 + 32) = roundup16(842) = 848;
    lds = rows_cap * (pitch + 64 * 3) + 4 * (64 * 17 + 16 * 17) = 78 * 1040 + 5440 = 86 560 B > 65 536 B."""
    assert E.lds_bytes((64, 132), (16, 33), 3, 3) == 78 * (848 + 192) + 4 * (64 * 17 + 16 * 17) == 86560
    got = _check_images('ks17_4x', 'whole', (0, 0, 33, 16), 0, 1)
    assert got.shape == (3, 3, 16, 33)
    _check_images('ks17_3p9x', 'whole', (0, 0, 33, 17), 1, 1)        # 85 520 B, flipped


@pytest.mark.parametrize("name", E.MASK_CASES)
@pytest.mark.parametrize("chans", E.MASK_CHANNELS)
@pytest.mark.parametrize("flip", [0, 1])
def test_masks_of_1_3_and_4_channels(name, chans, flip):
    fx = _fx()
    key = E.mask_key(name, chans)
    (rh, rw) = E.CASES[name][1]
    box = (0, 0, rw, rh)
    got = _run_mask(_three(fx[key]), (rw, rh), box, flip)
    assert np.array_equal(got[0], fx[E.mask_key(name, chans, flip)])
    for f in (1, 2):
        assert np.array_equal(got[f], P.mask_labels(_expected(key, f, (rw, rh), box, flip)))


@pytest.mark.parametrize("chans", [1, 4])
def test_mask_crop_boxes_and_narrow_outputs(chans):
    """The mask kernel's own store tail (uchar4 or bytes) and crop fill: boxes over every side, widths 1, 2, 3, 5."""
    key = E.mask_key('kt9', chans)
    frames = _three(_fx()[key])
    for label, box in E.boxes('kt9'):
        for flip in (0, 1):
            got = _run_mask(frames, (42, 31), box, flip)
            for f in range(3):
                want = P.mask_labels(_expected(key, f, (42, 31), box, flip))
                assert np.array_equal(got[f], want), (label, flip, f)


def test_mask_of_16_channels_after_a_larger_tile_of_another_kernel_form():
    """The widest mask the launch accepts.  A 4-channel mask at 4x (97 792 B of LDS, the 17-tap kernel) and then 16
    channels at kt9's geometry (93 120 B, the 9-tap kernel): a second kernel form above 64 KB, asked for after a larger
    size has been granted to another form."""
    assert 64 * 1024 < E.lds_bytes((61, 83), (31, 42), 16, 1) == 93120 < E.lds_bytes((64, 132), (16, 33), 4, 1) == 97792
    fx = _fx()
    big = _run_mask(_three(fx[E.mask_key('ks17_4x', 4)]), (33, 16), (0, 0, 33, 16), 0)
    assert np.array_equal(big[0], fx[E.mask_key('ks17_4x', 4, 0)])
    pick = np.random.default_rng(16).integers(0, len(E.MASK_VALUES), (61 // 6 + 1, 83 // 8 + 1, 16))
    src = np.repeat(np.repeat(np.asarray(E.MASK_VALUES, np.uint8)[pick], 6, 0), 8, 1)[:61, :83]
    frames = _three(src)
    got = _run_mask(frames, (42, 31), (-5, -3, 48, 33), 1)
    for f in range(3):
        want = P.mask_labels(P.transform(frames[f], (42, 31), (-5, -3, 48, 33), True))
        assert np.array_equal(got[f], want), f"frame {f}: {(got[f] != want).sum()} labels differ"


@pytest.mark.parametrize("name,label,flip", [('kt9', 'overhang', 0), ('kt9', 'overhang', 1), ('ks17_4x', 'whole', 0)])
def test_source_alignment_does_not_change_a_byte(name, label, flip):
    """Frames that start 0, 1, 7 and 15 bytes past a 16-byte boundary, 0xFF around them: the 16-byte staging loads pull
    neighbouring bytes into LDS, and a wrong (b0 & 15) or x0 would bring one into a border pixel."""
    box = dict(E.boxes(name))[label]
    first = _check_images(name, label, box, flip, 1, 0)
    for offset in (1, 7, 15):
        assert np.array_equal(_check_images(name, label, box, flip, 1, offset), first), f"offset {offset}"


PRE = dict(E.PRE_CONFIGS, four_x=(((16, 33), (64, 132), (0.0, 0.0)), ((33, 16), (0, 0, 33, 16))))


@pytest.mark.parametrize("name", list(PRE))
@pytest.mark.parametrize("flip", [False, True])
def test_image_preprocessor_at_odd_geometries(name, flip):
    from sgv3d_amd.preprocess import ImagePreprocessor
    (final_dim, hw, bot), (dims, crop) = PRE[name]
    pre = ImagePreprocessor({'final_dim': final_dim, 'bot_pct_lim': bot}, IMG_CONF, src_hw=hw, flip=flip, device=DEV)
    assert pre.resize_dims == dims and pre.crop == crop
    rng = np.random.default_rng(hw[0] * 7 + flip)
    src = rng.integers(0, 256, (2,) + hw + (3,), dtype=np.uint8)
    imgs, _ = pre(torch.from_numpy(src).to(DEV))
    got = imgs.cpu().numpy()
    assert got.shape == (2, 1, 1, 3) + final_dim
    for b in range(2):
        want = _norm(P.transform(src[b], dims, crop, flip), True)
        assert np.array_equal(got[b, 0, 0], want), f"frame {b}: {(got[b, 0, 0] != want).sum()} values differ"
    pick = rng.integers(0, len(E.MASK_VALUES), (2, hw[0] // 6 + 1, hw[1] // 8 + 1, 3))
    masks = np.repeat(np.repeat(np.asarray(E.MASK_VALUES, np.uint8)[pick], 6, 1), 8, 2)[:, :hw[0], :hw[1]]
    masks = np.ascontiguousarray(masks)
    lab = pre.mask(torch.from_numpy(masks).to(DEV)).cpu().numpy()
    for b in range(2):
        assert np.array_equal(lab[b, 0], P.mask_labels(P.transform(masks[b], dims, crop, flip)))


# ---- augment.hip: stages C and D at odd output sizes, the brightness rule on known answers

def _aug(name, img_conf=IMG_CONF):
    from sgv3d_amd.train_augment import TrainAugmenter
    (final_dim, hw, bot), _ = E.PRE_CONFIGS[name]
    return TrainAugmenter({'final_dim': final_dim, 'bot_pct_lim': bot}, img_conf, src_hw=hw, device=DEV), hw


def _mixed_params(hw, bright):
    c = (hw[1] // 2 + 1, hw[0] // 2 - 1)
    return _placed([True, True, False, False], [0.83, 1.21, 1.0, 1.0], [1.7, -2.2, 0.0, 0.0], [2, -3, 0, 0], [c] * 4,
                   bright, [0.83, 0.0, 0.41, 0.0])


@pytest.mark.parametrize("name", list(E.PRE_CONFIGS))
def test_augment_mixed_batch_at_odd_sizes(name):
    """(rectified, jittered) = (1, 1), (1, 0), (0, 1), (0, 0) in one call: planes of odd size (37 x 61), an output
    narrower than the 4-pixel store (23 x 3), 16 output rows above the image with ksize 11 (40 x 63)."""
    aug, hw = _aug(name)
    p = _mixed_params(hw, [True, False, True, False])
    rng = np.random.default_rng(hw[1])
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    base = (128 + 90 * np.sin(xx / 5.0 + yy / 3.0))[None, ..., None]
    src = np.clip(base + rng.integers(-60, 61, (4,) + hw + (3,)), 0, 255).astype(np.uint8)
    imgs, _ = aug(torch.from_numpy(src).to(DEV), p)
    got = imgs.cpu().numpy()
    assert got.shape == (4, 1, 1, 3) + aug.final_dim
    for i in range(4):
        want = _restated(src[i], p, i, aug)
        assert np.array_equal(got[i, 0, 0], want), f"frame {i}: {(got[i, 0, 0] != want).sum()} values differ"


@pytest.mark.parametrize("name", list(E.PRE_CONFIGS))
@pytest.mark.parametrize("chans", [1, 3])
def test_augment_mask_at_odd_sizes(name, chans):
    aug, hw = _aug(name)
    p = _mixed_params(hw, [False] * 4)
    pick = np.random.default_rng(hw[0] + chans).integers(0, len(E.MASK_VALUES), (4, hw[0] // 6 + 1, hw[1] // 8 + 1, chans))
    masks = np.repeat(np.repeat(np.asarray(E.MASK_VALUES, np.uint8)[pick], 6, 1), 8, 2)[:, :hw[0], :hw[1]]
    masks = np.ascontiguousarray(masks)
    got = aug.mask(torch.from_numpy(masks).to(DEV), p).cpu().numpy()
    assert got.shape == (4, 1) + aug.final_dim
    for i in range(4):
        img = masks[i]
        if p.ie[i]:
            K = np.eye(4)
            K[:2, 2] = p.center[i]
            img = R.intrin_extrin_transform(img, p.ratio[i], p.roll_deg[i], int(p.transform_pitch[i]), K)
        want = P.mask_labels(P.transform(img, aug.pre.resize_dims, aug.pre.crop, False))
        assert np.array_equal(got[i, 0], want), f"mask {i}: {(got[i, 0] != want).sum()} labels differ"


def _gray_frame(values):
    v = np.asarray(values, np.uint8).reshape(6, 61)
    return np.repeat(v[..., None], 3, 2)            # R = G = B: cv2's 8-bit gray is the value itself


def test_brightness_known_answers():
    """cv2.convertScaleAbs(img, 1, beta) with beta = u (100 - mean gray) clamped to +-50, on 6 x 61 frames whose mean is an
    integer: every tie of the rounding (to even), the reflection |x + beta| below -beta, both clamps, saturation at 255."""
    from sgv3d_amd.train_augment import TrainAugmenter
    ramp = np.arange(183)
    rest = np.full(359, 7)
    rest[:101] = 8
    low = np.concatenate([[205, 206, 230, 255, 49, 50, 51], rest])
    frames = [_gray_frame(np.tile(ramp, 2)),                               # mean 91, u 0.5: beta 4.5
              _gray_frame(np.tile(ramp + 60, 2)),                          # mean 151, u 0.5: beta -25.5
              _gray_frame(np.concatenate([ramp, np.full(183, 255)])),      # mean 173, u 0.5: beta -36.5, reflects x < 37
              _gray_frame(low), _gray_frame(low)]                          # mean 10, u 2 and -2: beta 50 and -50
    us = [0.5, 0.5, 0.5, 2.0, -2.0]
    means = [91, 151, 173, 10, 10]
    for f, m in zip(frames, means):
        assert R.gray_sum(f) == m * 366 and f[..., 0].astype(np.int64).sum() == m * 366

    def ties(x, half):                      # rint(|x + half|) for half = k + 0.5: the even one of the two neighbours
        a = np.floor(np.abs(x + half)).astype(np.int64)
        return a + (a & 1)

    x = [f[..., 0].astype(np.int64) for f in frames]
    closed = [ties(x[0], 4.5), ties(x[1], -25.5), ties(x[2], -36.5), np.minimum(x[3] + 50, 255), np.abs(x[4] - 50)]
    assert closed[0][0, 0] == 4 and closed[0][0, 1] == 6 and closed[2][0, 36] == 0 and closed[2][0, 0] == 36
    assert closed[2][0, 1] == 36 and closed[2][0, 37] == 0 and closed[2][0, 38] == 2 and closed[2][5, 60] == 218
    assert (x[3] >= 206).sum() >= 3 and (closed[3] == 255).sum() == 4 and closed[4].min() == 0

    aug = TrainAugmenter({'final_dim': (6, 61), 'bot_pct_lim': (0.0, 0.0)}, UNIT_CONF, src_hw=(6, 61), device=DEV)
    p = _placed([False] * 5, [1.0] * 5, [0.0] * 5, [0] * 5, [(30, 3)] * 5, [True] * 5, us)
    imgs, _ = aug(torch.from_numpy(np.stack(frames)).to(DEV), p)
    got = imgs.cpu().numpy()[:, 0, 0]
    for i in range(5):
        want = closed[i].astype(np.float32)
        for c in range(3):
            assert np.array_equal(got[i, c], want), f"frame {i} channel {c}: {(got[i, c] != want).sum()} values differ"
        assert np.array_equal(R.brightness(frames[i], us[i])[..., 0], closed[i].astype(np.uint8))
