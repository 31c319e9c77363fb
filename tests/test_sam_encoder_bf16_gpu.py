"""GPU: the SAM ViT encoder's bf16 mode (csrc/vit_bf16.hip, hip_ops.VIT_BF16) against float64.

Attention is compared with tests/vit_ref.py in float64 on the bf16 ``qkv`` widened exactly, with ``pad_qkv`` and both tables rounded
to bf16 first (what the kernel does on the way in), under a bar computed FROM THE INPUTS ONLY.  With u = 2^-24, u_b = 2^-8, per
output element d of a query row (T window slots, padding tokens included, hd the head dimension, w the float64 softmax weights):

    D_d      = sum_k w_k |v_kd - ref_d|                                                       the spread of V around the output
    E        = max_k [ (hd + 3) u (scale sum_c |q_c k_c| + sum_c |q_c R_h,c| + sum_c |q_c R_w,c|) + 2^-16 (|T_h| + |T_w|) ]
    |d out_d| <= 2 [ (2 E + 8 u + 2 u_b) D_d + (T + 8) u max_k |v_kd| ] + u_b |ref_d|

(2 E: a logit's error moves its weight relative to the others twice; 2 u_b: P is rounded to bf16 and the row sum adds the rounded
P, so the output stays a convex combination with weights off by 2 u_b relatively; the last term is the output's own rounding.)  The
outer 2 is the only slack.  Every case prints its worst observed ratio to the bar.
"""
import os

import numpy as np
import pytest
import torch

import vit_ref as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
UB = 2.0 ** -8
DEV = "cuda:0"
GUARD = 256          # bf16 values on either side of ``out``
BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _attn_inputs(b, h, w, nh, hd, window, seed, rel=True, pad=True):
    g = _gen(seed)
    qkv = torch.randn(b, h, w, 3 * nh * hd, generator=g).to(BF)
    padq = torch.randn(3 * nh * hd, generator=g) if pad else None
    rh = 0.2 * torch.randn(2 * window[0] - 1, hd, generator=g) if rel else None
    rw = 0.2 * torch.randn(2 * window[1] - 1, hd, generator=g) if rel else None
    return qkv, padq, rh, rw


def _launch(qkv, nh, window, padq, rh, rw):
    """One launch into a NaN-filled ``out`` between two guard bands; checks the bands, that every value was written and that a
    repeat launch gives the same bits."""
    from sgv3d_amd.layers.backbones.sam_encoder import vit_attention_bf16
    dev = lambda t: None if t is None else t.to(DEV)
    b, h, w, c3 = qkv.shape
    n = b * h * w * (c3 // 3)
    buf = torch.full((n + 2 * GUARD,), 1024.0, device=DEV, dtype=BF)
    out = buf[GUARD:GUARD + n].view(b, h, w, c3 // 3)
    out.fill_(float('nan'))
    args = (dev(qkv), nh, window, dev(padq), dev(rh), dev(rw))
    got = vit_attention_bf16(*args, out=out)
    torch.cuda.synchronize()
    assert got.dtype == BF and got.data_ptr() == out.data_ptr()
    first = out.clone()
    assert bool((buf[:GUARD] == 1024.0).all()) and bool((buf[GUARD + n:] == 1024.0).all()), "wrote outside out"
    assert not bool(torch.isnan(first).any()), "an output value was not written"
    out.fill_(float('nan'))
    vit_attention_bf16(*args, out=out)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int16), out.view(torch.int16)), "a repeat launch gave other bits"
    return first


def _reference_and_bar(qkv, nh, window, padq, rh, rw):
    """float64 on the device: the restatement's output on the operands the kernel sees, and the bar above, both as [B, H, W, C]."""
    rounded = lambda t: None if t is None else t.to(BF).to(DEV, torch.float64)
    qkv, padq, rh, rw = qkv.to(DEV, torch.float64), rounded(padq), rounded(rh), rounded(rw)
    b, h, w, c3 = qkv.shape
    hd = c3 // 3 // nh
    q, k, v, _ = V.split_windows(qkv, nh, window, padq)
    logits = V.window_logits(q, k, window, rh, rw)
    wts = torch.softmax(logits, dim=-1)                                                     # [..., Tq, T]
    del logits
    ref = wts @ v                                                                           # [..., Tq, hd]
    e = (hd + 3) * U * V.window_logits(q.abs(), k.abs(), window, None if rh is None else rh.abs(), None if rw is None else rw.abs())
    if rh is not None:
        zk = torch.zeros_like(k)
        e = e + 2.0 ** -16 * (V.window_logits(q, zk, window, rh, torch.zeros_like(rw)).abs()
                              + V.window_logits(q, zk, window, torch.zeros_like(rh), rw).abs())
    e = e.amax(-1, keepdim=True)                                                            # [..., Tq, 1]
    t = q.shape[-2]
    spread = torch.empty_like(ref)
    for d in range(hd):                                                                     # D_d, one d at a time: [..., Tq, T] stays one tensor
        spread[..., d] = (wts * (v[..., None, :, d] - ref[..., :, None, d]).abs()).sum(-1)
    bar = 2.0 * ((2.0 * e + 8.0 * U + 2.0 * UB) * spread + (t + 8) * U * v.abs().amax(-2, keepdim=True)) + UB * ref.abs()
    return V.merge_windows(ref, window, h, w), V.merge_windows(bar, window, h, w)


def _check(label, got, ref, bar):
    err = (got.to(DEV).double() - ref).abs()
    ratio = float((err / bar).max())
    print(f"\n[vit_attention_bf16] {label}: worst |error| / bar = {ratio:.3f}, max |error| = {float(err.max()):.3e}")
    assert ratio <= 1.0, f"{label}: error {ratio:.3f} x the bar"
    return ratio


# (label, B, H, W, window (0 = whole map), hd, heads)
SHAPES = [
    ("global 6x10 hd32", 2, 6, 10, 0, 32, 2),          # T = 60: under one key tile
    ("global 16x16 hd64", 2, 16, 16, 0, 64, 2),        # T = 256: four exact tiles
    ("global 17x17 hd80", 2, 17, 17, 0, 80, 2),        # T = 289: one key past a tile; hd 80's zero extension
    ("window 4 on 9x11 hd32", 2, 9, 11, 4, 32, 2),     # pads to 12 x 12: bias tokens on two edges
    ("window 7 on 5x5 hd32", 2, 5, 5, 7, 32, 2),       # window larger than the map
    ("window 14 on 28x28 hd64", 2, 28, 28, 14, 64, 2),  # 196 keys: the skipped trailing 32-key block
]
WORKLOAD = [
    ("global 64x64 hd64", 1, 64, 64, 0, 64, 1),        # 4096 keys
]
# beyond the issue's table, the remaining instantiations: 16 or 32 queries per wave (windows of at most 64 slots, or more) x
# 16-byte T_w reads (window width a multiple of 4) or 4-byte ones; and a ragged last tile (T = 99: 35 keys, both 32-key blocks live)
EXTRA = [
    ("global 7x9 hd80", 1, 7, 9, 0, 80, 2),             # 16 per wave, 4-byte
    ("window 7 on 9x9 hd64", 1, 9, 9, 7, 64, 2),        # 16 per wave, 4-byte
    ("window 8 on 10x9 hd64", 1, 10, 9, 8, 64, 2),      # 16 per wave, 16-byte
    ("window 8 on 9x9 hd80", 1, 9, 9, 8, 80, 2),        # 16 per wave, 16-byte
    ("global 9x11 hd32", 1, 9, 11, 0, 32, 2),           # 32 per wave, 4-byte
    ("global 8x12 hd32", 1, 8, 12, 0, 32, 2),           # 32 per wave, 16-byte
    ("global 12x12 hd80", 1, 12, 12, 0, 80, 2),         # 32 per wave, 16-byte
    ("window 9 on 10x10 hd64", 1, 10, 10, 9, 64, 2),    # 32 per wave, 4-byte, bias tokens
]


@pytest.mark.parametrize("case", SHAPES + WORKLOAD + EXTRA, ids=lambda c: c[0])
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


# ------------------------------------------------------------------------------------------------
# known answers, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [32, 64, 80])
def test_attention_dominant_key_returns_its_value_row_exactly(hip, hd):
    """A 12 x 8 global map (T = 96: a 64-key tile and one 32-key block of the next).  Query i and key i carry the same +-1 code word,
    the query's times a power of two: the logit of key i exceeds every other by at least 200, so every other weight underflows to 0,
    P is exactly the unit vector e_i, the sum is 1.0 and the output row is v[i] bit for bit -- for every i in one launch.  A key
    order of P that V's operand does not follow returns another key's row on almost every query."""
    nh, h, w = 2, 12, 8
    t = h * w
    g = _gen(100 + hd)
    code = (torch.randint(0, 2, (nh, t, hd), generator=g) * 2 - 1).double()
    gram = code @ code.transpose(-1, -2)                                    # [nh, t, t]: hd on the diagonal
    off = gram - hd * torch.eye(t, dtype=torch.float64)
    worst = float((hd - off.masked_fill(torch.eye(t, dtype=torch.bool), -hd)).min())       # smallest hd - s_i . s_j over i != j
    assert worst >= 2.0
    c = 2.0 ** int(np.ceil(np.log2(200.0 / (hd ** -0.5 * worst))))
    qkv = torch.zeros(1, t, 3, nh, hd)
    qkv[0, :, 0] = (c * code).permute(1, 0, 2)
    qkv[0, :, 1] = code.permute(1, 0, 2)
    qkv[0, :, 2] = torch.randn(t, nh, hd, generator=g)
    qkv = qkv.to(BF).view(1, h, w, 3 * nh * hd)
    q, k, _, _ = V.split_windows(qkv.double(), nh, (h, w))
    logits = V.window_logits(q, k, (h, w))[0, 0, 0]                         # [nh, t, t]
    eye = torch.eye(t, dtype=torch.bool)
    gap = logits.diagonal(dim1=-2, dim2=-1).unsqueeze(-1) - logits.masked_fill(eye, float('-inf'))
    assert float(gap.min()) >= 200.0
    got = _launch(qkv, nh, (h, w), None, None, None)
    want = qkv.view(1, h, w, 3, nh * hd)[:, :, :, 2].to(DEV)
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), "query i did not get v[i] exactly"


def _uniform_case(h, w, window, nh, hd, seed):
    """q = 0 everywhere (the padding token's too): every slot of a window has weight 1 / T.  v is integer-valued with, per window and
    channel, mean over the T slots (padding tokens included) an integer: the output must be that integer exactly."""
    g = _gen(seed)
    wh, ww = window
    ny, nx = -(-h // wh), -(-w // ww)
    t = wh * ww
    c = nh * hd
    pad = torch.zeros(3, c)
    pad[1] = torch.randn(c, generator=g)
    pad[2] = torch.randint(-30, 31, (c,), generator=g).float()
    qkv = torch.zeros(1, h, w, 3, c)
    qkv[..., 1, :] = torch.randn(1, h, w, c, generator=g)
    want = torch.zeros(1, h, w, c)
    for wy in range(ny):
        for wx in range(nx):
            hs, ws = slice(wy * wh, min((wy + 1) * wh, h)), slice(wx * ww, min((wx + 1) * ww, w))
            n_real = (hs.stop - hs.start) * (ws.stop - ws.start)
            assert n_real % 2 == 0 and t % n_real == 0
            half = torch.randint(-10, 11, (n_real // 2, c), generator=g).float()
            delta = torch.cat([half, -half])[torch.randperm(n_real, generator=g)]        # sums to zero per channel
            mshift = torch.randint(1, 4, (c,), generator=g).float()                      # the window's mean is pad_v + mshift:
            delta += (t // n_real) * mshift                                              # the real tokens carry the padding's share
            v = (pad[2] + delta).view(hs.stop - hs.start, ws.stop - ws.start, c)
            assert float(v.abs().max()) <= 256.0                                         # integers bf16 holds exactly
            qkv[0, hs, ws, 2] = v
            want[0, hs, ws] = pad[2] + mshift
    rh = 0.2 * torch.randn(2 * wh - 1, hd, generator=g)
    rw = 0.2 * torch.randn(2 * ww - 1, hd, generator=g)
    qkv = qkv.view(1, h, w, 3 * c)
    return qkv.to(BF), pad.view(-1), rh, rw, want


@pytest.mark.parametrize("case", [(16, 16, (16, 16), 64), (6, 6, (4, 4), 32), (6, 6, (4, 4), 80)],
                         ids=["global_16x16_hd64", "window_4_on_6x6_hd32", "window_4_on_6x6_hd80"])
def test_attention_uniform_weights_return_the_window_mean_exactly(hip, case):
    """The mean includes the padding tokens (window 4 on 6 x 6: 0, 8, 8 and 12 of a window's 16 slots) and excludes the masked tail
    slots of the key tile (48 of 64)."""
    h, w, window, hd = case
    nh = 2
    qkv, pad, rh, rw, want = _uniform_case(h, w, window, nh, hd, seed=200 + hd)
    ref = V.attention(qkv.double(), nh, window, pad.to(BF).double(), rh.to(BF).double(), rw.to(BF).double())
    assert float((ref - want.double()).abs().max()) <= 1e-12          # the construction itself
    got = _launch(qkv, nh, window, pad, rh, rw)
    assert torch.equal(got.float().cpu(), want), "the window mean did not come back exactly"


def test_attention_all_logits_far_below_zero(hip):
    """Every logit <= -50 (k a negative multiple of q's direction): a tail slot left at logit 0 instead of -inf would win."""
    nh, hd, h, w = 2, 32, 9, 9
    g = _gen(17)
    e = torch.randn(hd, generator=g)
    e = e / e.norm()
    qkv = torch.empty(1, h, w, 3, nh, hd)
    qkv[0, :, :, 0] = (20.0 + 5.0 * torch.rand(h, w, nh, 1, generator=g)) * e
    qkv[0, :, :, 1] = -(20.0 + 5.0 * torch.rand(h, w, nh, 1, generator=g)) * e
    qkv[0, :, :, 2] = torch.randn(h, w, nh, hd, generator=g)
    qkv = qkv.view(1, h, w, -1).to(BF)
    logits = V.window_logits(*V.split_windows(qkv.double(), nh, (h, w))[:2], (h, w))
    assert float(logits.max()) <= -50.0
    got = _launch(qkv, nh, (h, w), None, None, None)
    assert bool(torch.isfinite(got.float()).all())
    _check("all logits <= -50", got, *_reference_and_bar(qkv, nh, (h, w), None, None, None))


def test_attention_logits_of_300_stay_finite(hip):
    nh, hd, h, w = 2, 64, 10, 10
    qkv, _, rh, rw = _attn_inputs(1, h, w, nh, hd, (h, w), seed=19, pad=False)
    q, k, _, _ = V.split_windows(qkv.double(), nh, (h, w))
    peak = float(V.window_logits(q, k, (h, w), rh.to(BF).double(), rw.to(BF).double()).abs().max())
    qkv = qkv.float()
    qkv.view(1, h, w, 3, nh, hd)[:, :, :, 0] *= 300.0 / peak
    qkv = qkv.to(BF)
    q, k, _, _ = V.split_windows(qkv.double(), nh, (h, w))
    peak = float(V.window_logits(q, k, (h, w), rh.to(BF).double(), rw.to(BF).double()).abs().max())
    assert 250.0 <= peak <= 350.0
    got = _launch(qkv, nh, (h, w), None, rh, rw)
    assert bool(torch.isfinite(got.float()).all())


# ------------------------------------------------------------------------------------------------
# the small entries: bit-equal to the f32 entry followed by a cast
# ------------------------------------------------------------------------------------------------
def _layernorm_case(rows, c, offset, seed):
    from sgv3d_amd.layers.backbones.common import layernorm
    g = _gen(seed + rows + c)
    x = (torch.randn(rows, c, generator=g) + offset).float().to(DEV)
    w = (0.5 + torch.rand(c, generator=g)).to(DEV)
    b = (0.5 * torch.randn(c, generator=g)).to(DEV)
    buf = torch.full((rows * c + 2 * GUARD,), 1024.0, device=DEV, dtype=BF)
    out = buf[GUARD:GUARD + rows * c].view(rows, c)
    out.fill_(float('nan'))
    got = layernorm(x, w, b, 1e-6, out=out)
    want = layernorm(x, w, b, 1e-6).to(BF)
    torch.cuda.synchronize()
    assert got.dtype == BF
    assert bool((buf[:GUARD] == 1024.0).all()) and bool((buf[GUARD + rows * c:] == 1024.0).all()), "wrote outside y"
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(layernorm(x, w, b, 1e-6, out_dtype=BF).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("c", [8, 40, 768, 1280])
@pytest.mark.parametrize("rows", [1, 7, 4097])
def test_layernorm_bf16out_is_the_f32_entry_and_a_cast(hip, c, rows):
    _layernorm_case(rows, c, 0.0, seed=23)


def test_layernorm_bf16out_row_far_from_zero(hip):
    _layernorm_case(7, 768, 1e4, seed=29)


def test_gelu_bf16_is_the_f32_entry_and_a_cast_on_every_bit_pattern(hip):
    """All 65 536 bf16 values, NaNs and infinities included; and a count that is no multiple of 8 (the scalar tail)."""
    from sgv3d_amd.layers.backbones.common import gelu_
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).to(DEV)
    x = bits.view(BF)
    want = gelu_(x.float().clone()).to(BF)
    got = gelu_(x.clone())
    torch.cuda.synchronize()
    assert got.dtype == BF
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaNs must give NaN, and nothing else may"
    assert bool(torch.isnan(got[torch.isnan(x)]).all())
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    inf = torch.tensor([float('inf')], device=DEV)
    assert float(gelu_(inf.to(BF))) == float(gelu_(inf.clone())) == float('inf')
    for n in (1, 7, 13, 8 * 256 + 5):
        buf = torch.full((n + 16,), 1024.0, device=DEV, dtype=BF)
        xs = x[16000:16000 + n].clone()
        buf[8:8 + n] = xs                      # 16-byte aligned start
        gelu_(buf[8:8 + n])
        assert torch.equal(buf[8:8 + n].view(torch.int16), gelu_(xs.float()).to(BF).view(torch.int16))
        assert bool((buf[:8] == 1024.0).all()) and bool((buf[8 + n:] == 1024.0).all())


# ------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "sam_encoder.npz"))


@pytest.fixture(scope="module")
def yardstick():
    return np.load(os.path.join(GOLDEN, "sam_encoder_bf16.npz"))


@pytest.fixture
def modes():
    """Sets (MFMA_BF16, VIT_BF16) through the returned function; restores both."""
    from sgv3d_amd import hip_ops
    saved = (hip_ops.MFMA_BF16, hip_ops.VIT_BF16, hip_ops.MFMA_F32X3)

    def set_modes(bf16, vit):
        hip_ops.MFMA_BF16, hip_ops.VIT_BF16, hip_ops.MFMA_F32X3 = bf16, vit, False
    yield set_modes
    hip_ops.MFMA_BF16, hip_ops.VIT_BF16, hip_ops.MFMA_F32X3 = saved


def _fixture_model(fixture, wts=None):
    from functools import partial
    from sgv3d_amd.layers.backbones.sam_encoder import ImageEncoderViT
    cfg = V.FIXTURE_CFG
    model = ImageEncoderViT(img_size=cfg['img_size'], patch_size=cfg['patch_size'], embed_dim=cfg['embed_dim'], depth=cfg['depth'],
                            num_heads=cfg['num_heads'], out_chans=cfg['out_chans'], window_size=cfg['window_size'],
                            global_attn_indexes=cfg['global_attn_indexes'], use_rel_pos=True,
                            norm_layer=partial(torch.nn.LayerNorm, eps=cfg['eps']), final_dim=cfg['final_dim'],
                            downsample_factor=cfg['downsample_factor'])
    if wts is None:
        wts = {k[2:]: torch.from_numpy(fixture[k]) for k in fixture.files if k.startswith('w/')}
    model.load_state_dict(wts)
    return model.to(DEV).eval(), wts


class _EntrySpy:
    """Counts the calls of the three new C ABI entries."""
    NAMES = ("sgv3d_vit_attention_bf16", "sgv3d_layernorm_bf16out", "sgv3d_gelu_bf16")

    def __init__(self, lib):
        self.lib, self.calls, self.saved = lib, {n: 0 for n in self.NAMES}, {}

    def __enter__(self):
        for n in self.NAMES:
            fn = getattr(self.lib, n)
            self.saved[n] = fn

            def wrapper(*a, _fn=fn, _n=n):
                self.calls[_n] += 1
                return _fn(*a)
            setattr(self.lib, n, wrapper)
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.lib, n, fn)


def test_model_against_float64_within_the_autocast_yardstick(hip, fixture, yardstick, modes):
    """Max abs and relative L2 against the reference's float64 output: each at most 1.5 x what the reference's own bf16-autocast run
    shows (tests/golden/sam_encoder_bf16.npz)."""
    modes(True, True)
    model, _ = _fixture_model(fixture)
    with _EntrySpy(hip.load()) as spy:
        out = model(torch.from_numpy(fixture['input']).float().to(DEV))
    assert tuple(out.shape) == (2, 32, 13, 24) and out.dtype == torch.float32
    want = torch.from_numpy(fixture['out'])
    err = out.cpu().double() - want
    max_abs, rel_l2 = float(err.abs().max()), float(err.norm() / want.norm())
    y_abs, y_rel = float(yardstick['max_abs']), float(yardstick['rel_l2'])
    print(f"\n[sam encoder bf16] against float64: max abs {max_abs:.3e} = {max_abs / y_abs:.2f} x the autocast yardstick {y_abs:.3e}; "
          f"relative L2 {rel_l2:.3e} = {rel_l2 / y_rel:.2f} x {y_rel:.3e}")
    assert spy.calls == {"sgv3d_vit_attention_bf16": 2, "sgv3d_layernorm_bf16out": 4, "sgv3d_gelu_bf16": 2}
    assert max_abs <= 1.5 * y_abs and rel_l2 <= 1.5 * y_rel


def test_model_keeps_bf16_between_the_residual_adds_and_an_f32_stream(hip, fixture, modes, monkeypatch):
    from sgv3d_amd.layers.backbones import common, sam_encoder
    modes(True, True)
    model, _ = _fixture_model(fixture)
    seen = {"attn": [], "gelu": [], "ln": []}
    real_attn, real_gelu, real_ln = sam_encoder.vit_attention_bf16, common.gelu_, sam_encoder.layernorm

    def attn(qkv, *a, **kw):
        out = real_attn(qkv, *a, **kw)
        seen["attn"].append((qkv.dtype, out.dtype))
        return out

    def gelu(x):
        seen["gelu"].append(x.dtype)
        return real_gelu(x)

    def ln(x, *a, **kw):
        out = real_ln(x, *a, **kw)
        seen["ln"].append((x.dtype, out.dtype))
        return out
    monkeypatch.setattr(sam_encoder, "vit_attention_bf16", attn)
    monkeypatch.setattr(sam_encoder, "vit_attention", lambda *a, **kw: pytest.fail("the f32 attention ran in bf16 mode"))
    monkeypatch.setattr(common, "gelu_", gelu)
    monkeypatch.setattr(sam_encoder, "layernorm", ln)
    stream = []
    hooks = [b.register_forward_hook(lambda m, i, o: stream.append((i[0].dtype, o.dtype))) for b in model.blocks]
    hooks += [model.blocks[0].attn.register_forward_hook(lambda m, i, o: stream.append((torch.float32, o.dtype))),
              model.blocks[0].mlp.register_forward_hook(lambda m, i, o: stream.append((torch.float32, o.dtype)))]
    model(torch.from_numpy(fixture['input']).float().to(DEV))
    for hk in hooks:
        hk.remove()
    assert seen["attn"] == [(BF, BF)] * 2
    assert seen["gelu"] == [BF] * 2
    assert seen["ln"] == [(torch.float32, BF)] * 4
    assert len(stream) == 4 and all(s == (torch.float32, torch.float32) for s in stream), "the residual stream must stay f32"


def test_model_graph_replay_is_bit_identical(hip, fixture, modes):
    modes(True, True)
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


def test_model_uses_weights_loaded_later(hip, fixture, modes):
    """After load_state_dict the model gives the bits of a model BUILT from the new weights (nothing packed is stale)."""
    modes(True, True)
    model, wts = _fixture_model(fixture)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    first = model(x).clone()
    g = _gen(41)
    changed = {k: (v + 0.05 * torch.randn(v.shape, generator=g) if v.dim() > 1 else v.clone()) for k, v in wts.items()}
    model.load_state_dict(changed)
    second = model(x).clone()
    fresh, _ = _fixture_model(fixture, changed)
    assert torch.equal(second, fresh(x))
    assert float((second - first).abs().max()) > 1e-2


@pytest.mark.parametrize("bf16,vit", [(True, False), (False, True)], ids=["switch_off_in_bf16_mode", "switch_on_in_f32_mode"])
def test_model_without_the_mode_calls_none_of_the_new_entries(hip, fixture, modes, bf16, vit):
    modes(bf16, vit)
    model, _ = _fixture_model(fixture)
    with _EntrySpy(hip.load()) as spy:
        out = model(torch.from_numpy(fixture['input']).float().to(DEV))
    assert spy.calls == {n: 0 for n in _EntrySpy.NAMES}
    modes(bf16, False)
    fresh, _ = _fixture_model(fixture)
    assert torch.equal(out, fresh(torch.from_numpy(fixture['input']).float().to(DEV))), "the switch alone must change no bit"


def test_vit_b_runs_at_the_workload_shape(hip, modes):
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b
    modes(True, True)
    torch.manual_seed(43)
    model = build_sam_vit_b((864, 1536), 16).to(DEV).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == 'pos_embed' or 'rel_pos' in name:
                p.normal_(0.0, 0.02)
    assert all(b.bf16_mode() for b in model.blocks)
    out = model(torch.randint(0, 256, (1, 3, 576, 1024), device=DEV).float())
    assert tuple(out.shape) == (1, 256, 54, 96) and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all())
