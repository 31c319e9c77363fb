"""GPU: the preprocessing launch (csrc/preprocess.hip) bit-exact against Pillow's outputs (tests/golden/preprocess.npz) and
the numpy restatement (tests/preprocess_ref.py), fed into the model and into FramePipeline, captured in a graph, and its
argument checks."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import preprocess_ref as R
from sgv3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "preprocess.npz"))


def _pre(final_dim, src_hw, bot=(0.0, 0.0), flip=False, img_conf=IMG_CONF):
    from sgv3d_amd.preprocess import ImagePreprocessor
    return ImagePreprocessor({'final_dim': final_dim, 'bot_pct_lim': bot}, img_conf, src_hw=src_hw, flip=flip, device=DEV)


def _fixture_pre(d, name):
    conf = d[f'{name}_conf']
    src = d[f'{name}_src']
    return src, d[f'{name}_out'], _pre((int(conf[0]), int(conf[1])), src.shape[:2], (float(conf[2]), float(conf[3])),
                                       bool(conf[4]))


@pytest.mark.parametrize("name", ["dair", "odd_crop", "upscale", "flip"])
@pytest.mark.parametrize("to_rgb", [True, False])
def test_images_bit_exact_against_pillow(fixture, name, to_rgb):
    src, want, pre = _fixture_pre(fixture, name)
    pre.to_rgb = to_rgb
    frames = torch.from_numpy(np.stack([src, src[::-1].copy()])).to(DEV)       # two different frames in one launch
    imgs, ida = pre(frames)
    torch.cuda.synchronize()
    assert imgs.shape == (2, 1, 1, 3) + want.shape[:2] and imgs.dtype == torch.float32
    assert ida.shape == (2, 1, 1, 4, 4) and torch.equal(ida[1, 0, 0].cpu(), torch.from_numpy(pre.ida))
    exp0 = R.normalize(want, IMG_CONF['img_mean'], IMG_CONF['img_std'], to_rgb)
    assert np.array_equal(imgs[0, 0, 0].cpu().numpy(), exp0)
    exp1 = R.normalize(R.transform(src[::-1], pre.resize_dims, pre.crop, pre.flip), IMG_CONF['img_mean'],
                       IMG_CONF['img_std'], to_rgb)
    assert np.array_equal(imgs[1, 0, 0].cpu().numpy(), exp1)


def test_mask_bit_exact_against_pillow(fixture):
    src, want, pre = _fixture_pre(fixture, "mask")
    out = pre.mask(torch.from_numpy(np.stack([src, src])).to(DEV))
    assert out.shape == (2, 1) + want.shape and out.dtype == torch.uint8
    assert np.array_equal(out[0, 0].cpu().numpy(), want) and np.array_equal(out[1, 0].cpu().numpy(), want)
    one = pre.mask(torch.from_numpy(np.ascontiguousarray(src[..., :1])[None, None]).to(DEV))    # 1-channel mask, [B, N, H, W, C]
    assert np.array_equal(one[0, 0].cpu().numpy(), want)


@pytest.mark.parametrize("flip", [False, True])
def test_full_size_matches_restatement(flip):
    """1080x1920 -> 864x1536 (the shipped DAIR configs), two seeded frames in [B, S, N, H, W, 3] form."""
    rng = np.random.default_rng(7 + flip)
    src = rng.integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    pre = _pre((864, 1536), (1080, 1920), flip=flip)
    imgs, _ = pre(torch.from_numpy(src).to(DEV).view(2, 1, 1, 1080, 1920, 3))
    got = imgs.cpu().numpy()
    for b in range(2):
        want = R.normalize(R.transform(src[b], pre.resize_dims, pre.crop, flip), IMG_CONF['img_mean'], IMG_CONF['img_std'],
                           True)
        assert np.array_equal(got[b, 0, 0], want), f"frame {b}: {(got[b, 0, 0] != want).sum()} values differ"


@pytest.fixture(scope="module")
def small_model():
    from sgv3d_amd.models.bev_height import BEVHeight
    bc, hc = S.small_conf(depth=18)
    torch.manual_seed(0)
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 1)
    return bc, m.to(DEV)


def _frames(n, hw, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n,) + hw + (3,), dtype=np.uint8)).to(DEV)


def test_model_on_preprocessed_frames(small_model):
    bc, m = small_model
    hw = (160, 240)                                   # -> 192 x 128 at the DAIR ratio 0.8
    pre = _pre(bc['final_dim'], hw)
    frames = _frames(2, hw, 3)
    imgs, ida = pre(frames)
    want_imgs = torch.from_numpy(np.stack([R.normalize(R.transform(f, pre.resize_dims, pre.crop, False), IMG_CONF['img_mean'],
                                                       IMG_CONF['img_std'], True) for f in frames.cpu().numpy()]))
    assert torch.equal(imgs.cpu(), want_imgs.view(imgs.shape))
    mats = {k: v.to(DEV) for k, v in S.make_mats(2, scale=128 / 864).items()}
    mats['ida_mats'] = ida
    with torch.no_grad():
        got = m(imgs, mats)
        got = [{k: v.clone() for k, v in t[0].items()} for t in got]
        want = m(want_imgs.view(imgs.shape).to(DEV), mats)
    for t in range(len(want)):
        for k, v in want[t][0].items():
            torch.testing.assert_close(got[t][k], v, rtol=1e-5, atol=1e-5)


def test_graph_capture_replays_identically():
    pre = _pre((72, 128), (90, 160), flip=True)
    frames = _frames(3, (90, 160), 5)
    want, _ = pre(frames)
    static = frames.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pre(static)                                    # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, ida = pre(static)
    static.zero_()
    g.replay()
    torch.cuda.synchronize()
    zero, _ = pre(torch.zeros_like(frames))
    assert torch.equal(out, zero)
    static.copy_(frames)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(ida[0, 0, 0].cpu(), torch.from_numpy(pre.ida))


def test_frame_pipeline_with_preprocessing(small_model):
    """FramePipeline(..., preprocess=pre): uint8 frames in, the predictions of the float32-fed pipeline out."""
    from sgv3d_amd.pipeline import FramePipeline
    bc, m = small_model
    hw = (160, 240)
    pre = _pre(bc['final_dim'], hw)
    f0, f1 = _frames(1, hw, 11), _frames(1, hw, 12)
    mats = {k: v.to(DEV) for k, v in S.make_mats(1, scale=128 / 864).items()}
    i0, i1 = pre(f0)[0], pre(f1)[0]
    plain = FramePipeline(m, i0, mats, slots=2)
    want = []
    for x in (i0, i1):
        want.append({k: v.clone() for k, v in plain.result(plain.submit(x, mats))[3][0].items()})
    del plain
    pipe = FramePipeline(m, f0, mats, slots=2, preprocess=pre)
    assert pipe.use_graph and pipe.in_frames[0].dtype == torch.uint8
    got = []
    for f in (f0, f1):
        got.append({k: v.clone() for k, v in pipe.result(pipe.submit(f, mats))[3][0].items()})
    for g, w in zip(got, want):
        for k in w:
            torch.testing.assert_close(g[k], w[k], rtol=1e-5, atol=1e-5)


def test_rejects_bad_input():
    pre = _pre((72, 128), (90, 160))
    good = _frames(1, (90, 160), 1)
    with pytest.raises(ValueError, match="CUDA"):
        pre(good.cpu())
    with pytest.raises(ValueError, match="uint8"):
        pre(good.float())
    with pytest.raises(ValueError, match="built for 90x160"):
        pre(_frames(1, (100, 160), 1))
    with pytest.raises(ValueError, match="contiguous"):
        pre(good.transpose(1, 2))
    with pytest.raises(NotImplementedError):
        from sgv3d_amd.preprocess import ImagePreprocessor
        ImagePreprocessor({'final_dim': (72, 128)}, IMG_CONF, src_hw=(90, 160), rotate=-5.4, device=DEV)
