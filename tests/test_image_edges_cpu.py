"""CPU: the edge-geometry fixture (tests/golden/image_edges.npz, made by Pillow) against the numpy restatement
(tests/preprocess_ref.py) and against Pillow itself, the library's coefficient tables at every size pair of the fixture,
the LDS sizes that make the 4x cases the large-LDS path, the refusal of a tile above the LDS cap, ImagePreprocessor's
geometry at the three odd configurations the GPU tests use, and the rectification restatement against Pillow at those
sizes."""
import ctypes

import numpy as np
import pytest

import image_edges as E
import preprocess_ref as R
import train_augment_ref as A

RUNS = E.image_runs()
MASKS = [(n, c, f) for n in E.MASK_CASES for c in E.MASK_CHANNELS for f in (0, 1)]
PAIRS = sorted({p for (h, w), (rh, rw), *_ in E.CASES.values() for p in ((w, rw), (h, rh))})


@pytest.fixture(scope="module")
def fx():
    return E.load()


@pytest.fixture(scope="module")
def resized(fx):
    """name -> the restatement's resize of the case's source (computed once, never modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.resize(fx[f'{name}_src'], tuple(int(v) for v in fx[f'{name}_geom']))
            cache[name].setflags(write=False)
        return cache[name]
    return get


def test_fixture_holds_the_table(fx):
    for name, ((h, w), (rh, rw), _, _, _) in E.CASES.items():
        assert fx[f'{name}_src'].shape == (h, w, 3) and fx[f'{name}_src'].dtype == np.uint8
        assert fx[f'{name}_geom'].tolist() == [rw, rh]
        assert fx[f'{name}_boxes'].tolist() == [list(b) for _, b in E.boxes(name)]
    assert sum(k.endswith(('_f0', '_f1')) for k in fx.files) == len(RUNS) + len(MASKS)
    widths = {b[2] - b[0] for _, _, b, _ in RUNS}
    assert {1, 2, 3, 5, 61} <= widths and any(w % 4 for w in widths)
    assert (fx[E.out_key('white', 'whole', 0)] == 255).all()


@pytest.mark.parametrize("name,label,box,flip", RUNS, ids=[E.out_key(n, l, f) for n, l, _, f in RUNS])
def test_restatement_reproduces_fixture(fx, resized, name, label, box, flip):
    want = fx[E.out_key(name, label, flip)]
    got = R.crop(resized(name), box)
    got = np.ascontiguousarray(got[:, ::-1]) if flip else got
    assert got.dtype == want.dtype and np.array_equal(got, want)
    if label == 'whole' and not flip:
        dims = tuple(int(v) for v in fx[f'{name}_geom'])
        assert np.array_equal(R.transform(fx[f'{name}_src'], dims, box, False), want)


@pytest.mark.parametrize("name,chans,flip", MASKS)
def test_restatement_reproduces_mask_fixture(fx, name, chans, flip):
    (rh, rw) = E.CASES[name][1]
    src = fx[E.mask_key(name, chans)]
    assert src.shape[2] == chans and all((src[..., 0] == v).any() for v in (39, 40, 79, 80, 239, 240))
    got = R.mask_labels(R.transform(src, (rw, rh), (0, 0, rw, rh), bool(flip)))
    assert np.array_equal(got, fx[E.mask_key(name, chans, flip)])


@pytest.mark.parametrize("name", list(E.CASES))
def test_restatement_matches_pillow(fx, resized, name):
    Image = pytest.importorskip("PIL.Image")
    src = fx[f'{name}_src']
    dims = tuple(int(v) for v in fx[f'{name}_geom'])
    img = Image.fromarray(src).resize(dims, Image.BICUBIC)
    assert np.array_equal(resized(name), np.array(img))
    assert np.array_equal(R.resize(src[..., 1], dims), np.array(Image.fromarray(src[..., 1]).resize(dims, Image.BICUBIC)))
    for _, box in E.boxes(name):
        assert np.array_equal(R.crop(resized(name), box), np.array(img.crop(box)))


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_library_coefficients_equal_restatement(n_in, n_out):
    from sgv3d_amd.preprocess import resample_coeffs
    b, k = resample_coeffs(n_in, n_out)
    b2, k2 = R.coeffs(n_in, n_out)
    assert k.shape[1] == E.ksize(n_in, n_out)
    assert np.array_equal(b, b2) and np.array_equal(k, k2)


def test_lds_sizes_of_the_4x_cases():
    """launch()'s formula at the fixture's sizes: which cases leave the default 64 KB, and the one that is refused."""
    assert E.lds_bytes((64, 132), (16, 33), 3, 3) == 86560
    assert E.lds_bytes((67, 131), (17, 33), 3, 3) == 85520
    assert E.lds_bytes((64, 132), (16, 33), 4, 1) == 97792
    assert E.lds_bytes((64, 132), (16, 33), 8, 1) == 181408 > 160 * 1024
    for name in ('kt9', 'ks13_steps', 'aniso_a', 'aniso_b', 'identity', 'up10x', 'white'):
        assert E.lds_bytes(*E.CASES[name][:2], 3, 3) <= 64 * 1024


def test_tile_above_the_lds_cap_is_refused_without_gpu():
    """An 8-channel mask at 64x132 -> 16x33 needs 181 408 B of LDS.  launch() makes no HIP call before that check, so
    ordinary host buffers stand in for the device pointers: they are never read."""
    from sgv3d_amd import _lib
    from sgv3d_amd.preprocess import resample_coeffs
    lib = _lib.load()
    xb, xk = resample_coeffs(132, 33)
    yb, yk = resample_coeffs(64, 16)
    src = np.zeros(64 * 132 * 8, np.uint8)
    dst = np.full(16 * 33, 0xA5, np.uint8)
    rc = lib.sgv3d_preprocess_mask(1, 64, 132, 8, 16, 33, 0, 0, 16, 33, 0, xb.ctypes.data, xk.ctypes.data, 17,
                                   yb.ctypes.data, yk.ctypes.data, 17, src.ctypes.data, dst.ctypes.data, None)
    assert rc == -1
    msg = lib.sgv3d_last_error()
    assert b"tile needs" in msg and b"181408" in msg
    assert (dst == 0xA5).all()


@pytest.mark.parametrize("name", list(E.PRE_CONFIGS))
def test_preprocessor_geometry(name):
    from sgv3d_amd.input_contract import ida_resize_crop
    from sgv3d_amd.preprocess import ImagePreprocessor
    (final_dim, src_hw, bot), (dims, crop) = E.PRE_CONFIGS[name]
    img_conf = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)
    pre = ImagePreprocessor({'final_dim': final_dim, 'bot_pct_lim': bot}, img_conf, src_hw=src_hw, device='cpu')
    assert pre.resize_dims == dims and pre.crop == crop
    _, dims2, crop2, _, _ = ida_resize_crop(src_hw, final_dim, bot)
    assert (tuple(dims2), tuple(int(v) for v in crop2)) == (dims, crop)


@pytest.mark.parametrize("name", list(E.PRE_CONFIGS))
@pytest.mark.parametrize("ratio,roll,tp", [(0.83, 1.7, 2), (1.21, -2.2, -3)])
def test_rectification_restatement_matches_pillow(name, ratio, roll, tp):
    """The expected values of the GPU mixed-batch test come from train_augment_ref at odd source sizes: the same Pillow
    calls as the reference's img_intrin_extrin_transform (dataset/nusc_mv_det_dataset.py:94-110) give the same bytes."""
    Image = pytest.importorskip("PIL.Image")
    h, w = E.PRE_CONFIGS[name][0][1]
    src = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    K = np.eye(4)
    K[:2, 2] = (w // 2 + 1, h // 2 - 1)
    center = (w // 2 + 1, h // 2 - 1)
    (nw, nh), (ox, oy) = A.scale_offsets(h, w, ratio, center)
    img = Image.fromarray(src).resize((nw, nh), Image.LANCZOS)
    if ratio <= 1.0:
        canvas = Image.new('RGB', (w, h))
        canvas.paste(img, (-ox, -oy))
    else:
        canvas = img.crop((ox, oy, ox + w, oy + h))
    want = np.array(canvas.rotate(-roll, resample=Image.BICUBIC, center=center, translate=(0, tp)))
    assert np.array_equal(A.intrin_extrin_transform(src, ratio, roll, tp, K), want)
