"""GPU: the training adjoints of the SAM ViT encoder (csrc/vit_grad.hip, sgv3d_amd/vit_grad.py, sgv3d_amd/vit_train.py).

The float64 side is tests/vit_grad_ref.py (the backward formulas written out, no autograd).  The bar of every output tensor is
4 x the error of that restatement's own float32 CPU run on the same inputs, floored at 2^-21 max |value| -- the rule of the DiceLoss
tests; the 4 is there because a kernel and the CPU run sum in different orders.  Every comparison prints its worst ratio to the bar.

Every backward launch of this file goes through ``_backward``: outputs and workspace pre-filled with NaN between guard bands, the
bands checked, every element written, and a second launch into fresh NaN giving the same bits.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import vit_grad_cases as K
import vit_grad_ref as VG
import vit_ref as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
MARK = 12345.0


def _dev(t):
    return None if t is None else t.to(DEV)


class Banded:
    """A NaN-filled f32 tensor of ``shape`` between two guard bands."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), MARK, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(float('nan'))

    def check(self, what):
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == MARK).all()) and bool((self.buf[GUARD + n:] == MARK).all()), f"wrote outside {what}"
        assert not bool(torch.isnan(self.t).any()), f"an element of {what} was not written"


def _backward_once(lib, hip, d, qkv, pad, rh, rw, out, lse, dout):
    outs = dict(dqkv=Banded(qkv.shape), dpad=None if pad is None else Banded(pad.shape), drh=None if rh is None else Banded(rh.shape),
                drw=None if rw is None else Banded(rw.shape))
    nws = int(lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(d)))
    assert nws > 0 and nws % 4 == 0
    ws = Banded((nws // 4,))
    p = lambda b: None if b is None else b.t.data_ptr()
    rc = lib.sgv3d_vit_attention_backward(ctypes.byref(d), qkv.data_ptr(), hip.ptr(pad), hip.ptr(rh), hip.ptr(rw), out.data_ptr(), lse.data_ptr(),
                                          dout.data_ptr(), p(outs['dqkv']), p(outs['dpad']), p(outs['drh']), p(outs['drw']), ws.t.data_ptr(), nws,
                                          hip.stream_handle(DEV))
    hip.check(rc, "sgv3d_vit_attention_backward")
    torch.cuda.synchronize()
    for k, b in outs.items():
        if b is not None:
            b.check(k)
    n = ws.t.numel()
    assert bool((ws.buf[:GUARD] == MARK).all()) and bool((ws.buf[GUARD + n:] == MARK).all()), "wrote outside the workspace"
    return {k: None if b is None else b.t.clone() for k, b in outs.items()}


def _backward(hip, heads, window, qkv, pad, rh, rw, dout):
    """Forward with lse, then the backward twice under the launch hygiene above.  CPU float32 tensors in; device tensors out."""
    from sgv3d_amd import vit_grad
    lib = hip.load()
    qkv, pad, rh, rw, dout = (_dev(t) for t in (qkv, pad, rh, rw, dout))
    out, lse = vit_grad.attention_lse(qkv, heads, window, pad, rh, rw)
    b, h, w, c3 = qkv.shape
    d = hip.VitAttnDesc(b, h, w, heads, c3 // 3 // heads, window[0], window[1])
    first = _backward_once(lib, hip, d, qkv, pad, rh, rw, out, lse, dout)
    second = _backward_once(lib, hip, d, qkv, pad, rh, rw, out, lse, dout)
    for k, v in first.items():
        assert v is None or torch.equal(v, second[k]), f"a repeat launch gave other bits of {k}"
    first.update(out=out, lse=lse)
    return first


def _ratio(label, got, want, bar):
    err = float((got.double().cpu() - want).abs().max())
    ratio = err / bar if bar > 0.0 else (0.0 if err == 0.0 else float('inf'))      # a gradient that is exactly zero must come out so
    print(f"\n[vit_grad] {label}: max |error| {err:.3e}, bar {bar:.3e}, ratio {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_attention_lse_entry(hip, i):
    """``out`` bit-equal to sgv3d_vit_attention; lse against float64 under the 4 x rule."""
    from sgv3d_amd import vit_grad
    from sgv3d_amd.layers.backbones.sam_encoder import vit_attention
    c = K.CASES[i]
    qkv, pad, rh, rw, _ = (_dev(t) for t in K.inputs(i))
    out, lse = vit_grad.attention_lse(qkv, c['heads'], c['window'], pad, rh, rw)
    assert torch.equal(out, vit_attention(qkv, c['heads'], c['window'], pad, rh, rw))
    assert tuple(lse.shape) == (c['batch'], c['heads'], *c['hw'])
    assert _ratio(f"{K.IDS[i]} lse", lse, K.reference(i)['lse'], K.bars(i)['lse']) <= 1.0


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_attention_backward_against_float64(hip, i):
    c = K.CASES[i]
    got = _backward(hip, c['heads'], c['window'], *K.inputs(i))
    want, bars = K.reference(i), K.bars(i)
    worst = {}
    for k in ('dqkv', 'dpad', 'drh', 'drw'):
        if got[k] is not None:
            worst[k] = _ratio(f"{K.IDS[i]} {k}", got[k], want[k], bars[k])
    if c['pad']:
        assert float(got['dpad'][:c['heads'] * c['head_dim']].abs().max()) == 0.0, "the q part of dpad_qkv is exactly 0"
    assert all(r <= 1.0 for r in worst.values()), worst


# ---- known answers, bit for bit ----
def test_constant_v_gives_exactly_zero_dq_and_dk(hip):
    """v the same row for every key of a window: dP_ij = dO_i . v for every j, which is delta_i, so dS = 0.  For the equality to be
    exact in floating point the row is 0.5 in every channel (every channel of O then has the same bits) and dO_i = +-2^e
    alternating over the channels (dO_i . v and dO_i . O_i are both sums that cancel exactly)."""
    g = torch.Generator().manual_seed(3)
    nh, hd = 2, 64
    qkv = torch.randn(1, 8, 8, 3, nh, hd, generator=g)
    qkv[:, :, :, 2] = 0.5
    sign = torch.tensor([1.0, -1.0]).repeat(hd // 2)
    dout = (2.0 ** torch.randint(0, 3, (1, 8, 8, nh, 1), generator=g).float()) * sign
    rh, rw = 0.2 * torch.randn(7, hd, generator=g), 0.2 * torch.randn(7, hd, generator=g)
    got = _backward(hip, nh, (4, 4), qkv.reshape(1, 8, 8, -1), None, rh, rw, dout.reshape(1, 8, 8, -1).contiguous())
    dq, dk, dv = got['dqkv'].view(1, 8, 8, 3, nh, hd).unbind(3)
    assert float(dq.abs().max()) == 0.0 and float(dk.abs().max()) == 0.0
    assert float(dv.abs().max()) > 0.0
    assert float(got['drh'].abs().max()) == 0.0 and float(got['drw'].abs().max()) == 0.0


def test_zero_q_gives_the_window_mean_of_dout(hip):
    """q = 0, no tables, a 4 x 4 window on an 8 x 8 map: P = 1/16, so dv_j = (1/16) sum_i dO_i exactly for small-integer dO."""
    g = torch.Generator().manual_seed(4)
    nh, hd = 1, 32
    qkv = torch.randn(2, 8, 8, 3, nh, hd, generator=g)
    qkv[:, :, :, 0] = 0.0
    dout = torch.randint(-8, 9, (2, 8, 8, nh * hd), generator=g).float()
    got = _backward(hip, nh, (4, 4), qkv.reshape(2, 8, 8, -1), None, None, None, dout)
    dv = got['dqkv'].view(2, 8, 8, 3, nh * hd)[:, :, :, 2].cpu()
    want = dout.view(2, 2, 4, 2, 4, -1).sum((2, 4), keepdim=True).expand(2, 2, 4, 2, 4, -1).reshape(2, 8, 8, -1) / 16.0
    assert torch.equal(dv, want)


def test_dominant_key_takes_dout_exactly(hip):
    """Every query of the 12 x 12 global map has one key whose logit leads every other by at least 200 (>= 50; at 200 the others'
    P are exactly 0 whether or not denormals are kept, l = 1 and lse is the maximum): dv of a dominant key is the sum of dO over
    its queries, and every other dv is 0.  head_dim 64 (scale 1/8) and integer q, k make the recomputed logits exact."""
    hd, n = 64, 144
    q, k = torch.zeros(n, hd), torch.zeros(n, hd)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    hot = perm[:n // 2].repeat(2)                       # query i -> key hot[i]: two queries per dominant key, half of the keys nobody's
    for j in range(n):                                  # a key is a two-digit code, 80 at each digit
        k[j, j // 12] = 80.0
        k[j, 12 + j % 12] = 80.0
    for i in range(n):                                  # a query asks for its key's code: 200 per matching digit after the scale
        j = int(hot[i])
        q[i, j // 12] = 20.0
        q[i, 12 + j % 12] = 20.0
    g = torch.Generator().manual_seed(6)
    v = torch.randn(n, hd, generator=g)
    logits = (q * 0.125) @ k.t()
    top2 = logits.topk(2, dim=1).values
    assert bool((logits.argmax(1) == hot).all()) and float((top2[:, 0] - top2[:, 1]).min()) == 200.0
    dout = torch.randint(-8, 9, (n, hd), generator=g).float()
    qkv = torch.stack([q, k, v], 1).reshape(1, 12, 12, 3 * hd)
    got = _backward(hip, 1, (12, 12), qkv, None, None, None, dout.reshape(1, 12, 12, hd))
    dv = got['dqkv'].view(n, 3, hd)[:, 2].cpu()
    assert torch.equal(dv, torch.zeros(n, hd).index_add_(0, hot, dout))


def test_logits_of_300_give_finite_gradients(hip):
    g = torch.Generator().manual_seed(8)
    nh, hd = 1, 64
    qkv = torch.randn(1, 9, 8, 3, nh, hd, generator=g)
    qkv[:, :, :, 0] *= 100.0                            # scale q . k ~ N(0, 100^2): a few hundred at the ends
    pad = torch.randn(3 * hd, generator=g)
    dout = torch.randn(1, 9, 8, hd, generator=g)
    logits = V.window_logits(*V.split_windows(qkv.reshape(1, 9, 8, -1).double(), nh, (5, 5), pad.double())[:2], (5, 5))
    assert float(logits.max()) >= 300.0 and float(logits.min()) <= -300.0
    got = _backward(hip, nh, (5, 5), qkv.reshape(1, 9, 8, -1), pad, None, None, dout)
    assert bool(torch.isfinite(got['dqkv']).all()) and bool(torch.isfinite(got['dpad']).all())


def test_short_workspace_is_refused_before_any_launch(hip):
    lib = hip.load()
    c = K.CASES[0]
    qkv, pad, rh, rw, dout = (_dev(t) for t in K.inputs(0))
    from sgv3d_amd import vit_grad
    out, lse = vit_grad.attention_lse(qkv, c['heads'], c['window'], pad, rh, rw)
    d = hip.VitAttnDesc(c['batch'], *c['hw'], c['heads'], c['head_dim'], *c['window'])
    nws = int(lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(d)))
    outs = [Banded(t.shape) for t in (qkv, pad, rh, rw)]
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc = lib.sgv3d_vit_attention_backward(ctypes.byref(d), qkv.data_ptr(), pad.data_ptr(), rh.data_ptr(), rw.data_ptr(), out.data_ptr(),
                                          lse.data_ptr(), dout.data_ptr(), *(o.t.data_ptr() for o in outs), ws.data_ptr(), nws - 16,
                                          hip.stream_handle(DEV))
    torch.cuda.synchronize()
    assert rc == -3 and b"workspace" in lib.sgv3d_last_error()
    for o in outs:
        assert bool(torch.isnan(o.t).all()), "something was launched"


# ---- LayerNorm, GELU, resize ----
@pytest.mark.parametrize("rows", (1, 7, 4097))
@pytest.mark.parametrize("c", (4, 36, 768, 1280))
def test_layernorm_backward_against_float64(hip, c, rows):
    from sgv3d_amd import vit_grad
    g = torch.Generator().manual_seed(100 * c + rows)
    x = torch.randn(rows, c, generator=g) + torch.linspace(0.0, 1e4, rows).reshape(rows, 1)       # the rows sit at 0 .. 1e4
    w, dy = torch.rand(c, generator=g) + 0.5, torch.randn(rows, c, generator=g)
    want = VG.layernorm_backward(x.double(), w.double(), 1e-6, dy.double())
    f32 = VG.layernorm_backward(x, w, 1e-6, dy)
    got = vit_grad.layernorm_backward(_dev(x), _dev(w), 1e-6, _dev(dy))
    again = vit_grad.layernorm_backward(_dev(x), _dev(w), 1e-6, _dev(dy))
    torch.cuda.synchronize()
    worst = [_ratio(f"layernorm {rows} x {c} {n}", a, b, K.bar(f, b)) for n, a, b, f in zip(("dx", "dweight", "dbias"), got, want, f32)]
    for a, b in zip(got, again):
        assert torch.equal(a, b), "a repeat launch gave other bits"
    assert max(worst) <= 1.0, worst


def test_layernorm_backward_bands_and_aliasing(hip):
    lib = hip.load()
    rows, c = 7, 36
    g = torch.Generator().manual_seed(9)
    x, w, dy = _dev(torch.randn(rows, c, generator=g)), _dev(torch.rand(c, generator=g) + 0.5), _dev(torch.randn(rows, c, generator=g))
    dx, dw, db = Banded((rows, c)), Banded((c,)), Banded((c,))
    nws = int(lib.sgv3d_layernorm_backward_workspace_bytes(rows, c))
    ws = Banded((nws // 4,))
    call = lambda dx_ptr, dy_t, n=nws: lib.sgv3d_layernorm_backward(rows, c, x.data_ptr(), w.data_ptr(), ctypes.c_float(1e-6), dy_t.data_ptr(), dx_ptr,
                                                                   dw.t.data_ptr(), db.t.data_ptr(), ws.t.data_ptr(), n, hip.stream_handle(DEV))
    assert call(dx.t.data_ptr(), dy, nws - 8) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.t).all())
    hip.check(call(dx.t.data_ptr(), dy), "sgv3d_layernorm_backward")
    torch.cuda.synchronize()
    for b, n in ((dx, "dx"), (dw, "dweight"), (db, "dbias")):
        b.check(n)
    assert bool((ws.buf[:GUARD] == MARK).all()) and bool((ws.buf[GUARD + ws.t.numel():] == MARK).all())
    # dx on top of dy (or x) would feed dx to the weight and bias partials: refused by name, nothing launched
    kept = [b.t.clone() for b in (dx, dw, db)]
    for src in (dy, x):
        alias = src.clone()
        before = alias.clone()
        rc = lib.sgv3d_layernorm_backward(rows, c, (alias if src is x else x).data_ptr(), w.data_ptr(), ctypes.c_float(1e-6),
                                          (alias if src is dy else dy).data_ptr(), alias.data_ptr(), dw.t.data_ptr(), db.t.data_ptr(),
                                          ws.t.data_ptr(), nws, hip.stream_handle(DEV))
        torch.cuda.synchronize()
        assert rc == -1 and b"dx must not overlap x or dy" in lib.sgv3d_last_error()
        assert torch.equal(alias, before) and all(torch.equal(b.t, k) for b, k in zip((dx, dw, db), kept))


def test_gelu_backward_against_float64(hip):
    from sgv3d_amd import vit_grad
    g = torch.Generator().manual_seed(10)
    tiny = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 12.0, -12.0])      # 0 is where the forward changes from erfc to erf
    x = torch.cat([tiny, torch.linspace(-12, 12, 4001), 3.0 * torch.randn(1002, generator=g)])       # 5011 values: a tail of 3
    dy = torch.randn(x.shape, generator=g)
    want = VG.gelu_backward(x.double(), dy.double())
    band = Banded(x.shape)
    lib = hip.load()
    xd, dyd = _dev(x), _dev(dy)
    hip.check(lib.sgv3d_gelu_backward(x.numel(), xd.data_ptr(), dyd.data_ptr(), band.t.data_ptr(), hip.stream_handle(DEV)), "sgv3d_gelu_backward")
    torch.cuda.synchronize()
    band.check("dx")
    assert _ratio("gelu", band.t, want, K.bar(VG.gelu_backward(x, dy), want)) <= 1.0
    assert torch.equal(band.t, vit_grad.gelu_backward(xd, dyd))
    inplace = dyd.clone()
    hip.check(lib.sgv3d_gelu_backward(x.numel(), xd.data_ptr(), inplace.data_ptr(), inplace.data_ptr(), hip.stream_handle(DEV)), "sgv3d_gelu_backward")
    assert torch.equal(inplace, band.t)          # dx may be dy
    assert float(vit_grad.gelu_backward(_dev(torch.tensor([0.0, -0.0, 0.0, 0.0])), _dev(torch.ones(4)))[0]) == 0.5


@pytest.mark.parametrize("hw,crop,size", (((12, 12), (9, 16), (13, 24)), ((12, 10), (12, 10), (5, 3)), ((6, 7), (4, 5), (9, 11)),
                                         ((64, 64), (36, 64), (54, 96))), ids=("clamped-crop-up", "down", "crop-up", "vit-b"))
def test_resize_backward(hip, hw, crop, size):
    from sgv3d_amd import vit_grad
    from sgv3d_amd.layers.backbones.sam_encoder import resize_bilinear
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, *hw, 8, generator=g)
    dy = torch.randn(2, *size, 8, generator=g)
    band = Banded(x.shape)
    lib = hip.load()
    dyd = _dev(dy)
    hip.check(lib.sgv3d_resize_bilinear_backward(2, hw[0], hw[1], 8, crop[0], crop[1], size[0], size[1], dyd.data_ptr(), band.t.data_ptr(),
                                                 hip.stream_handle(DEV)), "sgv3d_resize_bilinear_backward")
    torch.cuda.synchronize()
    band.check("dx")
    want = VG.resize_bilinear_backward(dy.double(), hw, crop)
    assert _ratio("resize", band.t, want, K.bar(VG.resize_bilinear_backward(dy, hw, crop), want)) <= 1.0
    ch, cw = min(crop[0], hw[0]), min(crop[1], hw[1])
    outside = band.t.clone()
    outside[:, :ch, :cw] = 0.0
    assert float(outside.abs().max()) == 0.0, "rows and columns outside the crop are zero"
    # the adjoint identity with the forward kernel: both sides in f64 from f32 results that are each rounded once
    y = resize_bilinear(_dev(x), crop, size).double().cpu()
    lhs, rhs = (dy.double() * y), (band.t.double().cpu() * x.double())
    assert abs(float(lhs.sum() - rhs.sum())) <= 2.0 ** -24 * float(lhs.abs().sum() + rhs.abs().sum())
    assert torch.equal(band.t, vit_grad.resize_bilinear_backward(dyd, hw, crop))


# ---- module level ----
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
    model.load_state_dict({k[2:]: torch.from_numpy(fixture[k]) for k in fixture.files if k.startswith('w/')})
    return model.to(DEV)


def _grads(model, fn, x, cot):
    model.zero_grad(set_to_none=True)
    out = fn(model, x)
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("embed", (False, True), ids=("forward", "embed"))
def test_encoder_gradients_against_the_fixture(hip, fixture, embed):
    from sgv3d_amd import vit_train
    model = _fixture_model(fixture)
    fx = VG.open_fixture(GOLDEN, embed)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    cot = torch.from_numpy(fx['cot']).to(DEV)
    fn = vit_train.encoder_embed if embed else vit_train.encoder_forward
    out, grads = _grads(model, fn, x, cot)
    worst = {}
    for name, got in grads.items():
        want = VG.fixture_grad(fx, name)
        bar = max(4.0 * float(fx[f'ref_f32_grad_err/{name}']), 2.0 ** -21 * float(want.abs().max()))
        worst[name] = _ratio(f"{'embed' if embed else 'forward'} {name}", got, want, bar)
    assert max(worst.values()) <= 1.0, {k: round(v, 3) for k, v in worst.items() if v > 1.0}
    assert torch.equal(out, model.embed(x) if embed else model(x)), "the training forward gives other bits than the module"
    out2, grads2 = _grads(model, fn, x, cot)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads), "two eager runs differ"


def test_no_backward_entry_under_no_grad(hip, fixture, monkeypatch):
    from sgv3d_amd import vit_grad, vit_train
    model = _fixture_model(fixture)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    called = []
    for name in ("attention_lse", "attention_backward", "layernorm_backward", "gelu_backward", "resize_bilinear_backward"):
        monkeypatch.setattr(vit_grad, name, lambda *a, _n=name, **k: called.append(_n))
    with torch.no_grad():
        out = vit_train.encoder_forward(model, x)
    assert called == [] and torch.equal(out, model(x)) and not out.requires_grad
    for p in model.parameters():
        p.requires_grad_(False)
    out = vit_train.encoder_forward(model, x)                 # grad mode on, nothing to differentiate
    assert called == [] and not out.requires_grad


def test_uncovered_shape_raises_before_any_launch(hip, monkeypatch):
    """A head dimension outside hip_ops.vit_train_covers (48) on device tensors: raised by name, and no entry of the library is called."""
    from sgv3d_amd import _lib, hip_ops, vit_grad, vit_train
    from sgv3d_amd.layers.backbones.sam_encoder import Attention, Block, ImageEncoderViT
    assert not hip_ops.vit_train_covers(96, 2)
    enc = ImageEncoderViT(img_size=32, patch_size=8, embed_dim=96, depth=1, num_heads=2, out_chans=8).to(DEV)
    blk, attn = Block(96, 2).to(DEV), Attention(96, 2).to(DEV)
    img, tokens = torch.zeros(1, 3, 32, 32, device=DEV), torch.zeros(1, 4, 4, 96, device=DEV)
    torch.cuda.synchronize()
    called = []
    for name in ("attention", "attention_lse", "layer_norm", "gelu", "resize_bilinear"):
        monkeypatch.setattr(vit_grad, name, lambda *a, _n=name, **k: called.append(_n))
    monkeypatch.setattr(vit_train._PackedLayer, "apply", lambda *a, **k: called.append("packed layer"))
    monkeypatch.setattr(ImageEncoderViT, "batch_preprocess", lambda self, x: called.append("preprocess"))
    for fn, mod, x in ((vit_train.encoder_forward, enc, img), (vit_train.encoder_embed, enc, img), (vit_train.block_forward, blk, tokens),
                       (vit_train.attention_forward, attn, tokens)):
        with pytest.raises(_lib.SGV3DError, match="outside hip_ops.vit_train_covers"):
            fn(mod, x)
    assert called == []


def test_sgd_lowers_the_loss(hip, fixture):
    from sgv3d_amd import vit_train
    model = _fixture_model(fixture)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    with torch.no_grad():
        target = vit_train.encoder_forward(model, x) + 0.5
    opt = torch.optim.SGD(model.parameters(), lr=1e-6)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = ((vit_train.encoder_forward(model, x) - target) ** 2).sum()
        losses.append(float(loss))
        loss.backward()
        opt.step()
    print(f"\n[vit_train] SGD losses {losses}")
    assert losses[5] < losses[0], losses


def test_vit_b_full_size_backward_memory(hip):
    """ViT-B at [1, 3, 576, 1024]: finite gradients for all parameters, and the backward's peak stays below what one
    [12, 4096, 4096] float32 score tensor (805 MB) would add over the saved activations."""
    from sgv3d_amd import vit_train
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b
    torch.manual_seed(0)
    model = build_sam_vit_b((864, 1536), 16).to(DEV)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'rel_pos' in name or name == 'pos_embed':
                p.normal_(0.0, 0.02)
    x = 255.0 * torch.rand(1, 3, 576, 1024, device=DEV)
    out = vit_train.encoder_forward(model, x)
    assert tuple(out.shape) == (1, 256, 54, 96)
    cot = torch.randn_like(out)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    over = torch.cuda.max_memory_allocated() - held
    n_param = sum(p.numel() for p in model.parameters())
    print(f"\n[vit_train] ViT-B backward: saved activations {held / 1e6:.0f} MB, peak over them {over / 1e6:.0f} MB "
          f"(of which the gradients {4 * n_param / 1e6:.0f} MB)")
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert over < 12 * 4096 * 4096 * 4


def test_graph_capture_of_forward_and_backward(hip, fixture):
    from sgv3d_amd import vit_train
    model = _fixture_model(fixture)
    fx = VG.open_fixture(GOLDEN)
    cot = torch.from_numpy(fx['cot']).to(DEV)
    x0 = torch.from_numpy(fixture['input']).float().to(DEV)
    x1 = torch.flip(x0, dims=(0, 3)).contiguous()
    params = list(model.parameters())
    run = lambda x: torch.autograd.grad((vit_train.encoder_forward(model, x) * cot).sum(), params)
    run(x0)                                                   # first-call tile measurements happen outside the capture
    eager = [g.clone() for g in run(x1)]
    torch.cuda.synchronize()
    static = x0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(static)
    static.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
