"""GPU: the SAM ViT encoder's kernels (csrc/vit.hip) and module against float64.

Attention is compared with tests/vit_ref.py in float64 under a bar computed FROM THE INPUTS ONLY.  With u = 2^-24, per
query row of a window (T slots, padding tokens included, hd the head dimension):

    E        = max_k (hd + 3) u (scale sum_c |q_c k_c| + sum_c |q_c R_h,c| + sum_c |q_c R_w,c|)      the error of a logit
    |d out_d| <= 2 [ (2 E + 8 u) (max_k v_kd - min_k v_kd) + (T + 8) u max_k |v_kd| ]

(2 E: a logit's error moves its probability relative to the others twice, numerator and sum; 8 u: the exponential, the
rescales and the division; the last term: the f32 fma chain of P V over T keys.)  The outer 2 is the only slack.  Every
case prints its worst observed ratio to the bar.
"""
import os

import numpy as np
import pytest
import torch

import vit_ref as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DEV = "cuda:0"
GUARD = 256          # floats on either side of ``out``


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _attn_inputs(b, h, w, nh, hd, window, seed, rel=True, pad=True):
    g = _gen(seed)
    qkv = torch.randn(b, h, w, 3 * nh * hd, generator=g)
    padq = torch.randn(3 * nh * hd, generator=g) if pad else None
    rh = 0.2 * torch.randn(2 * window[0] - 1, hd, generator=g) if rel else None
    rw = 0.2 * torch.randn(2 * window[1] - 1, hd, generator=g) if rel else None
    return qkv, padq, rh, rw


def _launch(qkv, nh, window, padq, rh, rw):
    """One launch into a NaN-filled ``out`` between two guard bands; checks the bands and that every value was written."""
    from sgv3d_amd.layers.backbones.sam_encoder import vit_attention
    dev = lambda t: None if t is None else t.to(DEV)
    b, h, w, c3 = qkv.shape
    n = b * h * w * (c3 // 3)
    buf = torch.full((n + 2 * GUARD,), 12345.0, device=DEV)
    out = buf[GUARD:GUARD + n].view(b, h, w, c3 // 3)
    out.fill_(float('nan'))
    args = (dev(qkv), nh, window, dev(padq), dev(rh), dev(rw))
    vit_attention(*args, out=out)
    torch.cuda.synchronize()
    first = out.clone()
    assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + n:] == 12345.0).all()), "wrote outside out"
    assert not bool(torch.isnan(first).any()), "an output value was not written"
    out.fill_(float('nan'))
    vit_attention(*args, out=out)
    torch.cuda.synchronize()
    assert torch.equal(first, out), "a repeat launch gave other bits"
    return first


def _reference_and_bar(qkv, nh, window, padq, rh, rw):
    """float64 on the device: the restatement's output and the bar above, both as [B, H, W, C]."""
    d = lambda t: None if t is None else t.to(DEV, torch.float64)
    qkv, padq, rh, rw = d(qkv), d(padq), d(rh), d(rw)
    b, h, w, c3 = qkv.shape
    hd = c3 // 3 // nh
    ref = V.attention(qkv, nh, window, padq, rh, rw)
    q, k, v, _ = V.split_windows(qkv, nh, window, padq)
    absl = V.window_logits(q.abs(), k.abs(), window, None if rh is None else rh.abs(), None if rw is None else rw.abs())
    e = (hd + 3) * U * absl.amax(-1, keepdim=True)                                          # [..., Tq, 1]
    t = q.shape[-2]
    spread = (v.amax(-2, keepdim=True) - v.amin(-2, keepdim=True))                          # [..., 1, hd]
    bar = 2.0 * ((2.0 * e + 8.0 * U) * spread + (t + 8) * U * v.abs().amax(-2, keepdim=True))
    return ref, V.merge_windows(bar, window, h, w)


def _check(label, got, ref, bar):
    ratio = float(((got.double() - ref).abs() / bar).max())
    print(f"\n[vit_attention] {label}: worst |error| / bar = {ratio:.3f}, max |error| = {float((got.double() - ref).abs().max()):.3e}")
    assert ratio <= 1.0, f"{label}: error {ratio:.3f} x the bar"
    return ratio


# (label, B, H, W, window (0 = whole map), hd, heads)
SHAPES = [
    ("global 6x10 hd32", 2, 6, 10, 0, 32, 2),          # rectangular map, T = 60: less than one key tile
    ("global 16x16 hd64", 2, 16, 16, 0, 64, 2),        # T = 256: four exact tiles
    ("global 17x17 hd80", 2, 17, 17, 0, 80, 2),        # T = 289: one key past a tile
    ("window 4 on 9x11 hd32", 2, 9, 11, 4, 32, 2),     # pads to 12 x 12: bias tokens on two edges
    ("window 7 on 5x5 hd32", 2, 5, 5, 7, 32, 2),       # window larger than the map
    ("window 14 on 28x28 hd64", 2, 28, 28, 14, 64, 2),  # no padding
]
WORKLOAD = [
    ("global 64x64 hd64", 1, 64, 64, 0, 64, 1),        # 4096 keys
    ("window 14 on 64x64 hd64", 1, 64, 64, 14, 64, 2),  # pads to 70
]


@pytest.mark.parametrize("case", SHAPES + WORKLOAD, ids=lambda c: c[0])
def test_attention_against_float64(hip, case):
    label, b, h, w, win, hd, nh = case
    window = (win, win) if win else (h, w)
    args = _attn_inputs(b, h, w, nh, hd, window, seed=11)
    got = _launch(args[0], nh, window, *args[1:])
    _check(label, got, *_reference_and_bar(args[0], nh, window, *args[1:]))


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c[0])
def test_attention_without_rel_pos_and_with_zero_padding_tokens(hip, case):
    label, b, h, w, win, hd, nh = case
    window = (win, win) if win else (h, w)
    args = _attn_inputs(b, h, w, nh, hd, window, seed=12, rel=False, pad=False)
    got = _launch(args[0], nh, window, *args[1:])
    _check(label + " (no rel-pos, pad_qkv null)", got, *_reference_and_bar(args[0], nh, window, *args[1:]))


@pytest.mark.parametrize("hot", [0, 80, 63, 64], ids=["first", "last", "end_of_tile_0", "start_of_tile_1"])
def test_attention_one_dominant_key_returns_its_value_row_exactly(hip, hot):
    """A 9 x 9 map, T = 81 (a 64-key tile and 17 keys of the next).  Key ``hot`` has logit 10 hd^-0.5 120 = 212, every other key
    a logit within +-1: their exponentials underflow to 0, the sum is 1.0, and the output row is v[hot] bit for bit."""
    nh, hd, h, w = 2, 32, 9, 9
    g = _gen(13 + hot)
    qkv = torch.zeros(1, h, w, 3, nh, hd)
    qkv[..., 0, :, 0] = 10.0                                            # q = 10 e_0
    k = 0.02 * torch.randn(h * w, nh, hd, generator=g)
    k[hot, :, :] = 0.0
    k[hot, :, 0] = 120.0
    qkv[0, :, :, 1] = k.view(h, w, nh, hd)
    qkv[0, :, :, 2] = torch.randn(h, w, nh, hd, generator=g)
    got = _launch(qkv.view(1, h, w, -1), nh, (h, w), None, None, None)
    want = qkv[0, :, :, 2].reshape(h * w, nh * hd)[hot].to(DEV)
    assert torch.equal(got.view(h * w, -1), want.expand(h * w, -1)), "the dominant key's v row did not come back exactly"


def test_attention_all_logits_far_below_zero(hip):
    """Every logit <= -50 (k a negative multiple of q's direction): a tail slot left at logit 0 instead of -inf would win."""
    nh, hd, h, w = 2, 32, 9, 9
    g = _gen(17)
    e = torch.randn(hd, generator=g)
    e = e / e.norm()
    a = 20.0 + 5.0 * torch.rand(h, w, nh, 1, generator=g)
    qkv = torch.empty(1, h, w, 3, nh, hd)
    qkv[0, :, :, 0] = a * e
    qkv[0, :, :, 1] = -(20.0 + 5.0 * torch.rand(h, w, nh, 1, generator=g)) * e
    qkv[0, :, :, 2] = torch.randn(h, w, nh, hd, generator=g)
    qkv = qkv.view(1, h, w, -1)
    logits = V.window_logits(*V.split_windows(qkv.double(), nh, (h, w))[:2], (h, w))
    assert float(logits.max()) <= -50.0
    got = _launch(qkv, nh, (h, w), None, None, None)
    _check("all logits <= -50", got, *_reference_and_bar(qkv, nh, (h, w), None, None, None))


def test_attention_logits_of_300_stay_finite(hip):
    nh, hd, h, w = 2, 64, 10, 10
    qkv, _, rh, rw = _attn_inputs(1, h, w, nh, hd, (h, w), seed=19, pad=False)
    q, k, _, _ = V.split_windows(qkv.double(), nh, (h, w))
    peak = float(V.window_logits(q, k, (h, w), rh.double(), rw.double()).abs().max())
    qkv.view(1, h, w, 3, nh, hd)[:, :, :, 0] *= 300.0 / peak
    got = _launch(qkv, nh, (h, w), None, rh, rw)
    assert bool(torch.isfinite(got).all())
    _check("logits up to +-300", got, *_reference_and_bar(qkv, nh, (h, w), None, rh, rw))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 36, 768, 1280])
@pytest.mark.parametrize("rows", [1, 7, 4097])
def test_layernorm_against_float64(hip, c, rows):
    """Bar: 8 u (|x_hat| |w| (1 + |x|_max / sigma) + |b|), element by element (|x|_max and sigma per row)."""
    _layernorm_case(rows, c, 0.0, seed=23)


def test_layernorm_row_far_from_zero(hip):
    """Row mean 1e4, unit spread: E[x^2] - E[x]^2 has no correct digit here, and a mean rounded to f32 shifts every x_hat."""
    _layernorm_case(7, 768, 1e4, seed=29)


def _layernorm_case(rows, c, offset, seed):
    from sgv3d_amd.layers.backbones.common import layernorm
    g = _gen(seed + rows + c)
    x = (torch.randn(rows, c, generator=g) + offset).float()
    w = 0.5 + torch.rand(c, generator=g)
    b = 0.5 * torch.randn(c, generator=g)
    eps = 1e-6
    got = layernorm(x.to(DEV), w.to(DEV), b.to(DEV), eps).cpu().double()
    xd, wd, bd = x.double(), w.double(), b.double()
    mu = xd.mean(-1, keepdim=True)
    sigma = torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (xd - mu) / sigma
    ref = xhat * wd + bd
    bar = 8 * U * (xhat.abs() * wd.abs() * (1 + xd.abs().amax(-1, keepdim=True) / sigma) + bd.abs())
    ratio = float(((got - ref).abs() / bar).max())
    print(f"\n[layernorm] rows {rows} C {c} offset {offset:g}: worst |error| / bar = {ratio:.3f}")
    assert ratio <= 1.0


def test_gelu_against_float64(hip):
    """Bar: 4 x the worst error of torch's own float32 CPU gelu against float64 on the same inputs, plus u |y|."""
    from sgv3d_amd.layers.backbones.common import gelu_
    x = torch.cat([torch.linspace(-12.0, 12.0, 48001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0])])
    ref = torch.nn.functional.gelu(x.double())
    torch_err = float((torch.nn.functional.gelu(x).double() - ref).abs().max())
    got = gelu_(x.to(DEV).clone()).cpu().double()
    err = (got - ref).abs()
    print(f"\n[gelu] worst |error| {float(err.max()):.3e}; torch float32 CPU gelu on the same inputs {torch_err:.3e}")
    assert bool((err <= 4 * torch_err + U * ref.abs()).all())


def test_preprocess_against_float64(hip):
    from sgv3d_amd.layers.backbones.sam_encoder import vit_preprocess
    img = torch.randint(0, 256, (2, 3, 54, 96), generator=_gen(31)).float()
    mean = torch.tensor([123.675, 116.28, 103.53])
    std = torch.tensor([58.395, 57.12, 57.375])
    got = vit_preprocess(img.to(DEV), mean.to(DEV), std.to(DEV), 96).cpu()
    ref = V.preprocess(img.double(), mean.double(), std.double(), 96).permute(0, 2, 3, 1)
    assert tuple(got.shape) == (2, 96, 96, 4)
    assert float((got[..., :3].double() - ref).abs().max()) <= 4 * U * float(ref.abs().max())
    assert bool((got[..., 3] == 0).all()) and bool((got[:, 54:] == 0).all()), "the padding must be zero, not -mean / std"


@pytest.mark.parametrize("case", [(12, 12, 9, 16, 13, 24), (7, 5, 7, 5, 15, 11), (20, 18, 20, 18, 6, 7), (6, 9, 50, 50, 9, 6)],
                         ids=["fixture_crop_9x12_to_13x24", "upscale", "downscale", "crop_larger_than_map"])
def test_resize_bilinear_against_float64(hip, case):
    from sgv3d_amd.layers.backbones.sam_encoder import resize_bilinear
    h, w, ch, cw, oh, ow = case
    x = torch.randn(2, h, w, 8, generator=_gen(37))
    got = resize_bilinear(x.to(DEV), (ch, cw), (oh, ow)).cpu().double()
    ref = torch.nn.functional.interpolate(x.double().permute(0, 3, 1, 2)[:, :, :ch, :cw], (oh, ow), mode="bilinear",
                                          align_corners=False).permute(0, 2, 3, 1)
    assert float((got - ref).abs().max()) <= 4 * U * float(x.abs().max())


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "sam_encoder.npz"))


def _fixture_model(fixture):
    from functools import partial
    from sgv3d_amd.layers.backbones.sam_encoder import ImageEncoderViT
    cfg = V.FIXTURE_CFG
    model = ImageEncoderViT(img_size=cfg['img_size'], patch_size=cfg['patch_size'], embed_dim=cfg['embed_dim'], depth=cfg['depth'],
                            num_heads=cfg['num_heads'], out_chans=cfg['out_chans'], window_size=cfg['window_size'],
                            global_attn_indexes=cfg['global_attn_indexes'], use_rel_pos=True,
                            norm_layer=partial(torch.nn.LayerNorm, eps=cfg['eps']), final_dim=cfg['final_dim'],
                            downsample_factor=cfg['downsample_factor'])
    wts = {k[2:]: torch.from_numpy(fixture[k]) for k in fixture.files if k.startswith('w/')}
    model.load_state_dict(wts)
    return model.to(DEV).eval(), wts


def test_model_against_the_reference(hip, fixture):
    """The fixture model: the final output and every block's output within 1e-3 of the reference's float64 run."""
    model, _ = _fixture_model(fixture)
    blocks = []
    hooks = [b.register_forward_hook(lambda m, i, o: blocks.append(o.clone())) for b in model.blocks]
    out = model(torch.from_numpy(fixture['input']).float().to(DEV))
    for hk in hooks:
        hk.remove()
    assert tuple(out.shape) == (2, 32, 13, 24)
    worst = float((out.cpu().double() - torch.from_numpy(fixture['out'])).abs().max())
    per_block = [float((b.cpu().double() - torch.from_numpy(fixture[f'block{i}'])).abs().max()) for i, b in enumerate(blocks)]
    print(f"\n[sam encoder] max |device - float64 reference|: output {worst:.3e}, blocks {['%.3e' % e for e in per_block]}; "
          f"the reference's own float32 run: {float(fixture['ref_f32_err']):.3e}")
    assert len(per_block) == 2 and worst <= 1e-3 and max(per_block) <= 1e-3


def test_model_graph_replay_is_bit_identical(hip, fixture):
    model, _ = _fixture_model(fixture)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    eager = model(x).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = model(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager, captured)


def test_model_uses_weights_loaded_later(hip, fixture):
    model, wts = _fixture_model(fixture)
    x = torch.from_numpy(fixture['input']).float()
    first = model(x.to(DEV)).clone()
    g = _gen(41)
    changed = {k: (v + 0.05 * torch.randn(v.shape, generator=g) if v.dim() > 1 else v.clone()) for k, v in wts.items()}
    model.load_state_dict(changed)
    second = model(x.to(DEV))
    ref = V.encoder_forward(changed, V.FIXTURE_CFG, x.double())
    assert float((second.cpu().double() - ref).abs().max()) <= 1e-3
    assert float((second - first).abs().max()) > 1e-2


def test_vit_b_runs_at_the_workload_shape(hip):
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b
    torch.manual_seed(43)
    model = build_sam_vit_b((864, 1536), 16).to(DEV).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == 'pos_embed' or 'rel_pos' in name:
                p.normal_(0.0, 0.02)
    out = model(torch.randint(0, 256, (1, 3, 576, 1024), device=DEV).float())
    assert tuple(out.shape) == (1, 256, 54, 96)
    assert bool(torch.isfinite(out).all())
