"""GPU: training the SAM ViT encoder in bf16 mode (hip_ops.VIT_TRAIN_BF16): csrc/vit_grad_bf16.hip, the lse form of the bf16 attention
forward, sgv3d_layernorm_backward_bf16dy, sgv3d_gelu_backward_bf16 and the wiring of sgv3d_amd/vit_train.py.

The float64 side of the attention tests is tests/vit_grad_ref.py on the operands the kernel is given (bf16 qkv and dO widened
exactly, the f32 pad_qkv and tables).  The bar of an output tensor is 4 x the error of tests/vit_grad_bf16_ref.py's run with the
kernel's rounding points ON against its run with them OFF on the same inputs (the factor 4 is the project's rule: a kernel and a CPU
run sum in different orders), floored at 2^-9 max |gradient| for the bf16 dqkv (one bf16 rounding of the largest value) and at
2^-21 max |gradient| for the f32 outputs.  Every comparison prints its ratio to the bar.

Which case reaches which instantiation: the 28 cases of tests/vit_grad_cases.py go round head_dim 32 / 64 / 80 within every
geometry, so attn_bwd16_prep_kernel<32 | 64 | 80> and attn_bwd16_kernel<32 | 64 | 80, keys | queries> (the only templates of
csrc/vit_grad_bf16.hip) each run in at least nine cases, with and without tables and padding tokens (run-time arguments).  The lse
form of the forward has the forward's twelve instantiations (head_dim x 16 / 32 queries per wave x 16- / 4-byte T_w reads), which the
shapes of tests/test_sam_encoder_bf16_gpu.py, restated below, were chosen to reach.

Every backward launch goes through ``_backward``: outputs and workspace pre-filled with NaN between guard bands, the bands checked,
every element written, and a second launch into fresh NaN giving the same bits.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import vit_grad_bf16_ref as R
import vit_grad_cases as K
import vit_grad_ref as VG
import vit_ref as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
MARK = 12345.0
BF = torch.bfloat16


def _dev(t):
    return None if t is None else t.to(DEV)


class Banded:
    """A NaN-filled tensor of ``shape`` between two guard bands."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), MARK, device=DEV, dtype=dtype)      # (12345 rounds to a bf16 value and stays it)
        self.mark = float(self.buf[0])
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(float('nan'))

    def check(self, what):
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == self.mark).all()) and bool((self.buf[GUARD + n:] == self.mark).all()), f"wrote outside {what}"
        assert not bool(torch.isnan(self.t).any()), f"an element of {what} was not written"


def _backward_once(lib, hip, d, qkv, pad, rh, rw, out, lse, dout):
    outs = dict(dqkv=Banded(qkv.shape, BF), dpad=None if pad is None else Banded(pad.shape), drh=None if rh is None else Banded(rh.shape),
                drw=None if rw is None else Banded(rw.shape))
    nws = int(lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(d)))
    assert nws > 0 and nws % 4 == 0
    ws = Banded((nws // 4,))
    p = lambda b: None if b is None else b.t.data_ptr()
    rc = lib.sgv3d_vit_attention_bf16_backward(ctypes.byref(d), qkv.data_ptr(), hip.ptr(pad), hip.ptr(rh), hip.ptr(rw), out.data_ptr(),
                                               lse.data_ptr(), dout.data_ptr(), p(outs['dqkv']), p(outs['dpad']), p(outs['drh']), p(outs['drw']),
                                               ws.t.data_ptr(), nws, hip.stream_handle(DEV))
    hip.check(rc, "sgv3d_vit_attention_bf16_backward")
    torch.cuda.synchronize()
    for k, b in outs.items():
        if b is not None:
            b.check(k)
    n = ws.t.numel()
    assert bool((ws.buf[:GUARD] == MARK).all()) and bool((ws.buf[GUARD + n:] == MARK).all()), "wrote outside the workspace"
    return {k: None if b is None else b.t.clone() for k, b in outs.items()}


def _backward(hip, heads, window, qkv, pad, rh, rw, dout):
    """Forward with lse, then the backward twice under the launch hygiene above.  CPU tensors in (qkv, dout bf16); device tensors out."""
    from sgv3d_amd import vit_grad
    lib = hip.load()
    assert qkv.dtype == BF and dout.dtype == BF
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
    print(f"\n[vit_grad_bf16] {label}: max |error| {err:.3e}, bar {bar:.3e}, ratio {ratio:.3f}")
    return ratio


def _bar(rounded, want, bf16_out):
    return max(4.0 * float((rounded - want).abs().max()), (2.0 ** -9 if bf16_out else 2.0 ** -21) * float(want.abs().max()))


def _d(t):
    return None if t is None else t.double()


# ---- the lse entry ----
# (label, B, H, W, window (0 = whole map), hd, heads): the shapes of tests/test_sam_encoder_bf16_gpu.py (its SHAPES, WORKLOAD and
# EXTRA tables, fifteen rows), restated
LSE_SHAPES = [
    ("global 6x10 hd32", 2, 6, 10, 0, 32, 2), ("global 16x16 hd64", 2, 16, 16, 0, 64, 2), ("global 17x17 hd80", 2, 17, 17, 0, 80, 2),
    ("window 4 on 9x11 hd32", 2, 9, 11, 4, 32, 2), ("window 7 on 5x5 hd32", 2, 5, 5, 7, 32, 2),
    ("window 14 on 28x28 hd64", 2, 28, 28, 14, 64, 2), ("global 64x64 hd64", 1, 64, 64, 0, 64, 1),
    ("global 7x9 hd80", 1, 7, 9, 0, 80, 2), ("window 7 on 9x9 hd64", 1, 9, 9, 7, 64, 2), ("window 8 on 10x9 hd64", 1, 10, 9, 8, 64, 2),
    ("window 8 on 9x9 hd80", 1, 9, 9, 8, 80, 2), ("global 9x11 hd32", 1, 9, 11, 0, 32, 2), ("global 8x12 hd32", 1, 8, 12, 0, 32, 2),
    ("global 12x12 hd80", 1, 12, 12, 0, 80, 2), ("window 9 on 10x10 hd64", 1, 10, 10, 9, 64, 2),
]


@pytest.mark.parametrize("case", LSE_SHAPES, ids=lambda c: c[0])
def test_lse_entry(hip, case):
    """``out`` bit-equal to sgv3d_vit_attention_bf16; lse (natural-log units) against float64 under the 4 x rule."""
    from sgv3d_amd import vit_grad
    from sgv3d_amd.layers.backbones.sam_encoder import vit_attention_bf16
    label, b, h, w, win, hd, nh = case
    window = (win, win) if win else (h, w)
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(b, h, w, 3 * nh * hd, generator=g).to(BF)
    pad = torch.randn(3 * nh * hd, generator=g)
    rh, rw = 0.2 * torch.randn(2 * window[0] - 1, hd, generator=g), 0.2 * torch.randn(2 * window[1] - 1, hd, generator=g)
    args = (_dev(qkv), nh, window, _dev(pad), _dev(rh), _dev(rw))
    out, lse = vit_grad.attention_lse(*args)
    assert out.dtype == BF and lse.dtype == torch.float32 and tuple(lse.shape) == (b, nh, h, w)
    assert torch.equal(out.view(torch.int16), vit_attention_bf16(*args).view(torch.int16))
    # float64 on the device (the 4096-key row is [4096, 4096])
    run = lambda **kw: R.attention_forward(_dev(qkv).double(), nh, window, _dev(pad).double(), _dev(rh).double(), _dev(rw).double(), **kw)[1]
    want, rounded = run(), run(**R.ALL_ON)
    bar = max(4.0 * float((rounded - want).abs().max()), 2.0 ** -21 * float(want.abs().max()))
    assert _ratio(f"{label} lse", lse, want.cpu(), bar) <= 1.0


# ---- the attention backward against float64 ----
def _case16(i):
    qkv, pad, rh, rw, dout = K.inputs(i)
    return qkv.to(BF), pad, rh, rw, dout.to(BF)


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_attention_backward_against_float64(hip, i):
    c = K.CASES[i]
    qkv, pad, rh, rw, dout = _case16(i)
    got = _backward(hip, c['heads'], c['window'], qkv, pad, rh, rw, dout)
    a64 = (qkv.double(), c['heads'], c['window'], _d(pad), _d(rh), _d(rw), dout.double())
    want = dict(zip(('dqkv', 'dpad', 'drh', 'drw'), VG.attention_backward(*a64)))
    off = dict(zip(('dqkv', 'dpad', 'drh', 'drw'), R.attention_backward(*a64)))
    on = dict(zip(('dqkv', 'dpad', 'drh', 'drw'), R.attention_backward(*a64, **R.ALL_ON)))
    worst = {}
    for k in ('dqkv', 'dpad', 'drh', 'drw'):
        if got[k] is not None and not (k == 'dpad' and not c['pad']):
            assert float((off[k] - want[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max()))
            worst[k] = _ratio(f"{K.IDS[i]} {k}", got[k], want[k], _bar(on[k], want[k], k == 'dqkv'))
    if c['pad']:
        nq = c['heads'] * c['head_dim']
        assert float(got['dpad'][:nq].abs().max()) == 0.0, "the q part of dpad_qkv is exactly 0"
        if float(want['dpad'].abs().max()) == 0.0:      # no padding slot in this geometry: exactly zero in float64, exactly zero here
            assert float(got['dpad'].abs().max()) == 0.0
    assert all(r <= 1.0 for r in worst.values()), worst


# ---- known answers, bit for bit ----
def test_constant_v_gives_exactly_zero_dq_and_dk(hip):
    """v the same row for every key of a window: dP_ij = dO_i . v = delta_i for every j, so dS = 0.  v = 0.5 in every channel (O is
    then 0.5 bit for bit: sum of rounded P times 0.5 over that same sum) and dO_i = +-2^e alternating over the channels (dO_i . v and
    dO_i . O_i cancel exactly)."""
    g = torch.Generator().manual_seed(3)
    nh, hd = 2, 64
    qkv = torch.randn(1, 8, 8, 3, nh, hd, generator=g)
    qkv[:, :, :, 2] = 0.5
    sign = torch.tensor([1.0, -1.0]).repeat(hd // 2)
    dout = (2.0 ** torch.randint(0, 3, (1, 8, 8, nh, 1), generator=g).float()) * sign
    rh, rw = 0.2 * torch.randn(7, hd, generator=g), 0.2 * torch.randn(7, hd, generator=g)
    got = _backward(hip, nh, (4, 4), qkv.reshape(1, 8, 8, -1).to(BF), None, rh, rw, dout.reshape(1, 8, 8, -1).contiguous().to(BF))
    assert bool((got['out'].float() == 0.5).all())
    dq, dk, dv = got['dqkv'].float().view(1, 8, 8, 3, nh, hd).unbind(3)
    assert float(dq.abs().max()) == 0.0 and float(dk.abs().max()) == 0.0
    assert float(dv.abs().max()) > 0.0
    assert float(got['drh'].abs().max()) == 0.0 and float(got['drw'].abs().max()) == 0.0


def test_zero_q_gives_the_window_mean_of_dout(hip):
    """q = 0, no tables, a 4 x 4 window (16 slots) on an 8 x 8 map: P = 1/16 exactly (a bf16 value), so dv_j = (1/16) sum_i dO_i
    exactly for small-integer dO, and the sum (at most 16 x 8 = 128 in steps of 1/16) is a bf16 value."""
    g = torch.Generator().manual_seed(4)
    nh, hd = 1, 32
    qkv = torch.randn(2, 8, 8, 3, nh, hd, generator=g)
    qkv[:, :, :, 0] = 0.0
    dout = torch.randint(-1, 2, (2, 8, 8, nh * hd), generator=g).float()          # sums within +-16: sixteenths of them are bf16 values
    got = _backward(hip, nh, (4, 4), qkv.reshape(2, 8, 8, -1).to(BF), None, None, None, dout.to(BF))
    dv = got['dqkv'].float().view(2, 8, 8, 3, nh * hd)[:, :, :, 2].cpu()
    want = dout.view(2, 2, 4, 2, 4, -1).sum((2, 4), keepdim=True).expand(2, 2, 4, 2, 4, -1).reshape(2, 8, 8, -1) / 16.0
    assert torch.equal(dv, want)


def _dominant(hd=64, n=144):
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
    return q, k, hot


def test_dominant_key_takes_dout_exactly(hip):
    """Every query of the 12 x 12 global map has one key whose logit leads every other by 200: the others' P are exactly 0, l = 1,
    P of the dominant key is exp2 of a difference below 2^-9, which rounds to the bf16 value 1.  dv of a dominant key is the sum of dO
    over its (two) queries, every other dv is 0; v a power of two makes dP = delta exactly, so dq = dk = 0."""
    hd, n = 64, 144
    q, k, hot = _dominant(hd, n)
    g = torch.Generator().manual_seed(6)
    v = 2.0 ** torch.randint(-2, 3, (n, 1), generator=g).float() * torch.ones(n, hd)
    logits = (q * 0.125) @ k.t()
    top2 = logits.topk(2, dim=1).values
    assert bool((logits.argmax(1) == hot).all()) and float((top2[:, 0] - top2[:, 1]).min()) == 200.0
    dout = torch.randint(-8, 9, (n, hd), generator=g).float()
    qkv = torch.stack([q, k, v], 1).reshape(1, 12, 12, 3 * hd).to(BF)
    got = _backward(hip, 1, (12, 12), qkv, None, None, None, dout.reshape(1, 12, 12, hd).to(BF))
    dq, dk, dv = got['dqkv'].float().view(n, 3, hd).cpu().unbind(1)
    assert torch.equal(got['out'].float().view(n, hd).cpu(), v[hot])
    assert torch.equal(dv, torch.zeros(n, hd).index_add_(0, hot, dout))
    assert float(dq.abs().max()) == 0.0 and float(dk.abs().max()) == 0.0


def test_padding_slots_are_keys_and_never_queries(hip):
    """A 3 x 3 map in one 4 x 4 window: 7 padding slots.  q = 0 and no tables make P = 1/16 over all 16 slots, so every real key's dv
    is (1/16) of the sum of dO over the NINE real queries (padding slots present as keys: the 1/16; absent as queries: nine terms), and
    dpad_qkv's v part is 7 x that row."""
    nh, hd = 1, 32
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(1, 3, 3, 3, nh, hd, generator=g)
    qkv[:, :, :, 0] = 0.0
    pad = torch.randn(3 * hd, generator=g)
    pad[:hd] = 0.0
    dout = torch.randint(-1, 2, (1, 3, 3, hd), generator=g).float()
    got = _backward(hip, nh, (4, 4), qkv.reshape(1, 3, 3, -1).to(BF), pad, None, None, dout.to(BF))
    row = dout.sum((0, 1, 2)) / 16.0
    dv = got['dqkv'].float().view(9, 3, hd)[:, 2].cpu()
    assert torch.equal(dv, row.expand(9, hd))
    assert torch.equal(got['dpad'][2 * hd:].cpu(), 7.0 * row)
    assert float(got['dpad'][:hd].abs().max()) == 0.0


# ---- robustness ----
def test_logits_of_300_give_finite_gradients(hip):
    g = torch.Generator().manual_seed(8)
    nh, hd = 1, 64
    qkv = torch.randn(1, 9, 8, 3, nh, hd, generator=g)
    qkv[:, :, :, 0] *= 100.0                            # scale q . k ~ N(0, 100^2): a few hundred at the ends
    pad = torch.randn(3 * hd, generator=g)
    dout = torch.randn(1, 9, 8, hd, generator=g)
    q16 = qkv.reshape(1, 9, 8, -1).to(BF)
    logits = V.window_logits(*V.split_windows(q16.double(), nh, (5, 5), R.bf16(pad.double()))[:2], (5, 5))
    assert float(logits.max()) >= 300.0 and float(logits.min()) <= -300.0
    got = _backward(hip, nh, (5, 5), q16, pad, None, None, dout.to(BF))
    assert bool(torch.isfinite(got['dqkv'].float()).all()) and bool(torch.isfinite(got['dpad']).all()) and bool(torch.isfinite(got['lse']).all())


def test_all_logits_below_minus_50_give_finite_gradients(hip):
    """q = -k direction: every logit of the global 8 x 9 map is at most -50; the row maximum keeps P away from underflow."""
    nh, hd = 1, 32
    g = torch.Generator().manual_seed(9)
    base = torch.ones(hd) * 4.0
    q = -(base + 0.25 * torch.rand(72, hd, generator=g))
    k = base + 0.25 * torch.rand(72, hd, generator=g)
    v, dout = torch.randn(72, hd, generator=g), torch.randn(72, hd, generator=g)
    qkv = torch.stack([q, k, v], 1).reshape(1, 8, 9, 3 * hd).to(BF)
    logits = (qkv.view(72, 3, hd)[:, 0].double() * hd ** -0.5) @ qkv.view(72, 3, hd)[:, 1].double().t()
    assert float(logits.max()) <= -50.0
    got = _backward(hip, nh, (8, 9), qkv, None, None, None, dout.reshape(1, 8, 9, hd).to(BF))
    assert bool(torch.isfinite(got['dqkv'].float()).all()) and float(got['dqkv'].float().abs().max()) > 0.0


def test_workspace_one_byte_short_is_refused_before_any_launch(hip):
    from sgv3d_amd import vit_grad
    lib = hip.load()
    c = K.CASES[0]
    qkv, pad, rh, rw, dout = (_dev(t) for t in _case16(0))
    out, lse = vit_grad.attention_lse(qkv, c['heads'], c['window'], pad, rh, rw)
    d = hip.VitAttnDesc(c['batch'], *c['hw'], c['heads'], c['head_dim'], *c['window'])
    nws = int(lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(d)))
    outs = [Banded(qkv.shape, BF)] + [Banded(t.shape) for t in (pad, rh, rw)]
    ws = Banded((nws // 4,))
    rc = lib.sgv3d_vit_attention_bf16_backward(ctypes.byref(d), qkv.data_ptr(), pad.data_ptr(), rh.data_ptr(), rw.data_ptr(), out.data_ptr(),
                                               lse.data_ptr(), dout.data_ptr(), *(o.t.data_ptr() for o in outs), ws.t.data_ptr(), nws - 1,
                                               hip.stream_handle(DEV))
    torch.cuda.synchronize()
    assert rc == -3 and b"workspace" in lib.sgv3d_last_error()
    for o in outs + [ws]:
        assert bool(torch.isnan(o.t).all()), "something was launched"


# ---- the two thin adjoints: identities, not tolerances ----
@pytest.mark.parametrize("rows", (1, 7, 4097))
@pytest.mark.parametrize("c", (4, 36, 768, 1280))
def test_layernorm_backward_bf16dy_is_the_f32_entry_on_the_widened_dy(hip, c, rows):
    from sgv3d_amd import vit_grad
    g = torch.Generator().manual_seed(100 * c + rows)
    x = _dev(torch.randn(rows, c, generator=g) + torch.linspace(0.0, 1e4, rows).reshape(rows, 1))
    w, dy = _dev(torch.rand(c, generator=g) + 0.5), _dev(torch.randn(rows, c, generator=g).to(BF))
    lib = hip.load()
    outs = [Banded((rows, c)), Banded((c,)), Banded((c,))]
    nws = int(lib.sgv3d_layernorm_backward_workspace_bytes(rows, c))
    ws = Banded((nws // 4,))
    hip.check(lib.sgv3d_layernorm_backward_bf16dy(rows, c, x.data_ptr(), w.data_ptr(), ctypes.c_float(1e-6), dy.data_ptr(),
                                                  *(o.t.data_ptr() for o in outs), ws.t.data_ptr(), nws, hip.stream_handle(DEV)),
              "sgv3d_layernorm_backward_bf16dy")
    torch.cuda.synchronize()
    for o, n in zip(outs, ("dx", "dweight", "dbias")):
        o.check(n)
    assert bool((ws.buf[:GUARD] == MARK).all()) and bool((ws.buf[GUARD + ws.t.numel():] == MARK).all())
    want = vit_grad.layernorm_backward(x, w, 1e-6, dy.float())
    again = vit_grad.layernorm_backward(x, w, 1e-6, dy)
    for o, a, b in zip(outs, want, again):
        assert torch.equal(o.t, a) and torch.equal(o.t, b)


def test_gelu_backward_bf16_on_every_bf16_pattern(hip):
    """All 65 536 patterns of x with three dy: the f32 entry on the widened inputs followed by one cast, bit for bit (NaN patterns of
    x give NaN both ways: compared as bits after the cast, payloads aside); and in place."""
    from sgv3d_amd import vit_grad
    lib = hip.load()
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).to(DEV)
    for dyv in (1.0, -0.37109375, 3.0e4):
        dy = torch.full((65536,), dyv, dtype=BF, device=DEV)
        band = Banded((65536,), BF)
        hip.check(lib.sgv3d_gelu_backward_bf16(65536, x.data_ptr(), dy.data_ptr(), band.buf[GUARD:].data_ptr(), hip.stream_handle(DEV)),
                  "sgv3d_gelu_backward_bf16")
        torch.cuda.synchronize()
        got = band.t
        assert bool((band.buf[:GUARD] == band.mark).all()) and bool((band.buf[GUARD + 65536:] == band.mark).all())
        want = vit_grad.gelu_backward(x.float(), dy.float()).to(BF)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
        assert torch.equal(vit_grad.gelu_backward(x, dy).view(torch.int16)[~nan], want.view(torch.int16)[~nan])
        for alias in ("x", "dy"):
            xs, ds = x.clone(), dy.clone()
            dst = xs if alias == "x" else ds
            hip.check(lib.sgv3d_gelu_backward_bf16(65536, xs.data_ptr(), ds.data_ptr(), dst.data_ptr(), hip.stream_handle(DEV)), "in place")
            assert torch.equal(dst.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    # a tail that is no multiple of 8
    xs, ds = x[:5011].clone(), torch.full((5011,), 0.5, dtype=BF, device=DEV)
    assert torch.equal(vit_grad.gelu_backward(xs, ds).view(torch.int16)[:128], vit_grad.gelu_backward(xs.float(), ds.float()).to(BF).view(torch.int16)[:128])
    assert torch.equal(vit_grad.gelu_backward(xs, ds).view(torch.int16)[5000:5011],
                       vit_grad.gelu_backward(xs.float(), ds.float()).to(BF).view(torch.int16)[5000:5011])


# ---- module level ----
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "sam_encoder.npz"))


@pytest.fixture
def bf16_train(monkeypatch):
    """The switch on, in the compute mode it needs; the module forward's bf16 mode stays as it is unless a test turns it on."""
    from sgv3d_amd import hip_ops
    monkeypatch.setattr(hip_ops, "MFMA_BF16", True)
    monkeypatch.setattr(hip_ops, "MFMA_F32X3", False)
    monkeypatch.setattr(hip_ops, "TRAIN_BF16_WGRAD", True)
    monkeypatch.setattr(hip_ops, "VIT_TRAIN_BF16", True)
    return hip_ops


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


class Spy:
    """Counts the calls of the library's entries (every wrapper of the package calls ``_lib.load().<entry>``)."""

    def __init__(self, hip, monkeypatch, names):
        self.calls = {n: 0 for n in names}
        lib = hip.load()
        for n in names:
            real = getattr(lib, n)

            def wrapped(*a, _n=n, _real=real):
                self.calls[_n] += 1
                return _real(*a)
            monkeypatch.setattr(lib, n, wrapped)


BF16_ENTRIES = ("sgv3d_vit_attention_bf16_lse", "sgv3d_vit_attention_bf16_backward", "sgv3d_layernorm_backward_bf16dy",
                "sgv3d_gelu_backward_bf16")
F32_ENTRIES = ("sgv3d_vit_attention_lse", "sgv3d_vit_attention_backward", "sgv3d_gelu_backward")


@pytest.mark.parametrize("embed", (False, True), ids=("forward", "embed"))
def test_encoder_in_bf16_training_mode(hip, fixture, bf16_train, monkeypatch, embed):
    """The forward's bits are the module's with VIT_BF16 on; every parameter gradient within max(2 x the reference's own bf16-autocast
    error, 2^-21 max |gradient|) of float64 in both measures tests/golden/sam_encoder_grad_bf16.npz stores; the bf16 entries ran and
    the f32 attention adjoint did not; the saved tensors between the residual adds are bf16; two eager runs give the same bits."""
    from sgv3d_amd import vit_train
    model = _fixture_model(fixture)
    fx = VG.open_fixture(GOLDEN, embed)
    auto = np.load(os.path.join(GOLDEN, "sam_encoder_grad_bf16.npz"))
    run = 'embed' if embed else 'forward'
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    cot = torch.from_numpy(fx['cot']).to(DEV)
    fn = vit_train.encoder_embed if embed else vit_train.encoder_forward
    spy = Spy(hip, monkeypatch, BF16_ENTRIES + F32_ENTRIES)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((t.dtype, tuple(t.shape))), t)[1], lambda t: t):
        out, grads = _grads(model, fn, x, cot)
    depth = V.FIXTURE_CFG['depth']
    assert spy.calls["sgv3d_vit_attention_bf16_lse"] == depth and spy.calls["sgv3d_vit_attention_bf16_backward"] == depth
    assert spy.calls["sgv3d_layernorm_backward_bf16dy"] == 2 * depth and spy.calls["sgv3d_gelu_backward_bf16"] == depth
    assert all(spy.calls[n] == 0 for n in F32_ENTRIES), spy.calls
    dim, mlp = V.FIXTURE_CFG['embed_dim'], 4 * V.FIXTURE_CFG['embed_dim']
    inner = [dt for dt, shape in saved if len(shape) == 4 and shape[-1] in (3 * dim, mlp)]       # qkv, lin1's output
    assert len(inner) >= 3 * depth and all(dt == BF for dt in inner), "qkv and the MLP's hidden map are saved as bf16"
    monkeypatch.setattr(bf16_train, "VIT_BF16", True)
    assert torch.equal(out, model.embed(x) if embed else model(x)), "the training forward gives other bits than the module in bf16 mode"
    worst = {}
    for name, got in grads.items():
        want = VG.fixture_grad(fx, name)
        floor = 2.0 ** -21 * float(want.abs().max())
        r_abs = _ratio(f"{run} {name} max-abs", got, want, max(2.0 * float(auto[f'{run}/max_abs/{name}']), floor))
        rel = float((got.double().cpu() - want).norm() / want.norm())
        bar = max(2.0 * float(auto[f'{run}/rel_l2/{name}']), 2.0 ** -21)
        print(f"[vit_grad_bf16] {run} {name} rel-L2 {rel:.3e}, bar {bar:.3e}, ratio {rel / bar:.3f}")
        worst[name] = max(r_abs, rel / bar)
    assert max(worst.values()) <= 1.0, {k: round(v, 3) for k, v in worst.items() if v > 1.0}
    out2, grads2 = _grads(model, fn, x, cot)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads), "two eager runs differ"


def test_block_forward_bits_in_bf16_training_mode(hip, fixture, bf16_train, monkeypatch):
    from sgv3d_amd import vit_train
    model = _fixture_model(fixture)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 12, 12, V.FIXTURE_CFG['embed_dim'], generator=g).to(DEV)
    outs = [vit_train.block_forward(blk, x.clone().requires_grad_(True)).detach() for blk in model.blocks]
    monkeypatch.setattr(bf16_train, "VIT_BF16", True)
    for blk, o in zip(model.blocks, outs):
        assert torch.equal(o, blk(x))


def test_switch_off_is_the_f32_training_path_bit_for_bit(hip, fixture, monkeypatch):
    """Whatever the compute mode: with VIT_TRAIN_BF16 off the encoder's outputs and gradients are those of the f32 entries called
    directly, and no new entry is called."""
    from sgv3d_amd import hip_ops, vit_grad, vit_train
    assert not hip_ops.VIT_TRAIN_BF16
    fx = VG.open_fixture(GOLDEN)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    cot = torch.from_numpy(fx['cot']).to(DEV)
    # the two ways the rule is not met with the switch on: not the bf16 compute mode; the bf16 compute mode without bf16 weight gradients
    for mfma_bf16, wgrad in ((False, True), (True, False)):
        monkeypatch.setattr(hip_ops, "MFMA_BF16", mfma_bf16)
        monkeypatch.setattr(hip_ops, "MFMA_F32X3", False)
        monkeypatch.setattr(hip_ops, "TRAIN_BF16_WGRAD", wgrad)
        monkeypatch.setattr(hip_ops, "VIT_TRAIN_BF16", False)
        model = _fixture_model(fixture)
        out_off, grads_off = _grads(model, vit_train.encoder_forward, x, cot)
        assert torch.equal(out_off, model(x))
        monkeypatch.setattr(hip_ops, "VIT_TRAIN_BF16", True)
        assert not hip_ops.vit_train_bf16_active(64, 2, 256)
        spy = Spy(hip, monkeypatch, BF16_ENTRIES)
        out_un, grads_un = _grads(model, vit_train.encoder_forward, x, cot)
        assert all(v == 0 for v in spy.calls.values())
        assert torch.equal(out_off, out_un) and all(torch.equal(grads_off[k], grads_un[k]) for k in grads_off)
    # one attention, by hand through the f32 entries
    monkeypatch.setattr(hip_ops, "MFMA_BF16", False)
    monkeypatch.setattr(hip_ops, "TRAIN_BF16_WGRAD", True)
    monkeypatch.setattr(hip_ops, "VIT_TRAIN_BF16", False)
    blk = model.blocks[0]
    g = torch.Generator().manual_seed(22)
    y = torch.randn(2, 12, 12, 3 * V.FIXTURE_CFG['embed_dim'], generator=g).to(DEV).requires_grad_(True)
    dout = torch.randn(2, 12, 12, V.FIXTURE_CFG['embed_dim'], generator=g).to(DEV)
    a = blk.attn
    o = vit_grad.attention(y, a.num_heads, (5, 5), a.qkv.bias, a.rel_pos_h, a.rel_pos_w)
    got = torch.autograd.grad(o, (y, a.qkv.bias, a.rel_pos_h, a.rel_pos_w), dout)
    out, lse = vit_grad.attention_lse(y.detach(), a.num_heads, (5, 5), a.qkv.bias.detach(), a.rel_pos_h.detach(), a.rel_pos_w.detach())
    want = vit_grad.attention_backward(y.detach(), a.num_heads, (5, 5), a.qkv.bias.detach(), a.rel_pos_h.detach(), a.rel_pos_w.detach(), out, lse, dout)
    assert torch.equal(o.detach(), out) and all(torch.equal(p, q) for p, q in zip(got, want))


def test_no_entry_runs_under_no_grad(hip, fixture, bf16_train, monkeypatch):
    from sgv3d_amd import vit_train
    model = _fixture_model(fixture)
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    spy = Spy(hip, monkeypatch, BF16_ENTRIES + F32_ENTRIES)
    with torch.no_grad():
        out = vit_train.encoder_forward(model, x)
    assert all(v == 0 for v in spy.calls.values()) and not out.requires_grad
    for p in model.parameters():
        p.requires_grad_(False)
    out2 = vit_train.encoder_forward(model, x)                 # grad mode on, nothing to differentiate
    assert all(v == 0 for v in spy.calls.values()) and not out2.requires_grad and torch.equal(out, out2)


def test_uncovered_head_dim_keeps_the_f32_path(hip, bf16_train, monkeypatch):
    """A head dimension outside 32 / 64 / 80 is outside vit_train_covers too and raises before any launch, switch or no switch
    (tests/test_vit_grad_gpu.py).  The fall-back that can run is a Block the bf16 kernels do not take but the training forward does:
    an MLP width that is no multiple of 8 (44).  With the switch on it runs the f32 path: no bf16 entry, the f32 path's bits."""
    from sgv3d_amd import vit_train
    from sgv3d_amd.layers.backbones.sam_encoder import Block
    torch.manual_seed(3)
    blk = Block(64, 2, mlp_ratio=0.6875, use_rel_pos=True, window_size=0, input_size=(6, 6)).to(DEV)        # mlp_dim 44
    assert blk.mlp.lin1.out_features == 44
    assert not bf16_train.vit_train_bf16_active(64, 2, 44) and bf16_train.vit_train_covers(64, 2)
    with torch.no_grad():
        blk.attn.rel_pos_h.normal_(0.0, 0.1), blk.attn.rel_pos_w.normal_(0.0, 0.1)
    x = torch.randn(1, 6, 6, 64, device=DEV)
    spy = Spy(hip, monkeypatch, BF16_ENTRIES)

    def run():
        blk.zero_grad(set_to_none=True)
        o = vit_train.block_forward(blk, x)
        o.square().sum().backward()
        return o.detach(), [p.grad.clone() for p in blk.parameters()]
    on = run()
    assert all(v == 0 for v in spy.calls.values())
    monkeypatch.setattr(bf16_train, "VIT_TRAIN_BF16", False)
    off = run()
    assert torch.equal(on[0], off[0]) and all(torch.equal(a, b) for a, b in zip(on[1], off[1]))


def test_graph_capture_of_forward_and_backward(hip, fixture, bf16_train):
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


def test_sgd_follows_the_f32_path(hip, fixture, bf16_train, monkeypatch):
    """Six SGD steps lower the loss and end within 2 % of the f32-tensor training path's loss (the bar of the BEV mixed-precision test)."""
    from sgv3d_amd import vit_train
    x = torch.from_numpy(fixture['input']).float().to(DEV)
    ends = {}
    for mode in (True, False):
        monkeypatch.setattr(bf16_train, "VIT_TRAIN_BF16", mode)
        model = _fixture_model(fixture)
        with torch.no_grad():
            monkeypatch.setattr(bf16_train, "VIT_TRAIN_BF16", False)
            target = vit_train.encoder_forward(model, x) + 0.5
            monkeypatch.setattr(bf16_train, "VIT_TRAIN_BF16", mode)
        opt = torch.optim.SGD(model.parameters(), lr=1e-6)
        losses = []
        for _ in range(6):
            opt.zero_grad(set_to_none=True)
            loss = ((vit_train.encoder_forward(model, x) - target) ** 2).sum()
            losses.append(float(loss))
            loss.backward()
            opt.step()
        print(f"\n[vit_train bf16={mode}] SGD losses {losses}")
        assert losses[5] < losses[0], losses
        ends[mode] = losses[5]
    assert abs(ends[True] - ends[False]) <= 0.02 * ends[False], ends


def test_vit_b_full_size_peak_is_below_the_f32_path(hip, bf16_train, monkeypatch):
    """ViT-B at [1, 3, 576, 1024]: finite gradients, and the peak allocation over forward + backward is smaller than the f32 training
    path's in the same process."""
    from sgv3d_amd import vit_train
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b
    torch.manual_seed(0)
    model = build_sam_vit_b((864, 1536), 16).to(DEV)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'rel_pos' in name or name == 'pos_embed':
                p.normal_(0.0, 0.02)
    x = 255.0 * torch.rand(1, 3, 576, 1024, device=DEV)
    peaks = {}
    for mode in (False, True):
        monkeypatch.setattr(bf16_train, "VIT_TRAIN_BF16", mode)
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = vit_train.encoder_forward(model, x)
        out.square().sum().backward()
        torch.cuda.synchronize()
        peaks[mode] = torch.cuda.max_memory_allocated() - base
        del out
        if mode:
            for name, p in model.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    print(f"\n[vit_train] ViT-B forward + backward peak: f32 path {peaks[False] / 1e6:.0f} MB, bf16 mode {peaks[True] / 1e6:.0f} MB")
    assert peaks[True] < peaks[False]
