"""float64 restatements of the small inference layers of csrc/misc_layers.hip (and their bf16 twins in csrc/act_bf16.hip),
in the kernels' own NHWC layout, written from the definition of each operation and not from torch.nn.functional
(tests/test_small_layers_cpu.py pins each one against F.* in float64).  tests/test_small_layers_gpu.py compares the kernels
with them.

Every function has a ``magnitude=True`` form: the same computation on absolute values.  It is the ``S`` of the bound
``|got - want| <= (n + 2) 2^-24 S`` (n roundings on the kernel's longest path) the GPU file states its tolerances in.

The input generators of both test files live here too, so that what the CPU file proves about the reference ("exact for
integer inputs", "at most 1 % of the pixels near the threshold") is proved for the very tensors the GPU file uses.
"""
import math

import numpy as np
import torch

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
# Error of the device expf, relative to its result.  The ROCm device-library documentation is not shipped with the
# toolchain, so this is an ASSUMPTION: 2 ulp = 2 * 2^-23 = 4 * 2^-24, counted as four roundings.
EXPF_ROUNDINGS = 4
# 1 / (1 + expf(-v)): expf, the add, the divide.  expf's relative error enters with the factor e / (1 + e) <= 1.
SIGMOID_ROUNDINGS = EXPF_ROUNDINGS + 2
F32_TINY = 2.0 ** -126            # below the smallest normal f32 a relative bound says nothing (expf overflow, flushes)


# ------------------------------------------------------------------------------------------------------------ bf16
def round_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), returned as float64.  One rounding: torch's double -> bfloat16
    conversion goes through float32 and rounds twice.  (Finite values of normal bf16 magnitude, zeros, infinities.)"""
    a = np.ascontiguousarray(x.detach().cpu().to(F64).numpy())
    bits = a.view(np.int64)
    drop = 52 - 7                                              # bf16 keeps 7 fraction bits
    out = (bits + ((1 << (drop - 1)) - 1) + ((bits >> drop) & 1)) & ~((1 << drop) - 1)
    out = np.where(np.isnan(a), bits, out)
    return torch.from_numpy(out.view(np.float64).copy()).reshape(x.shape)


def is_bf16(x):
    """every element is a bf16 value"""
    x = x.to(F64)
    return bool(torch.equal(round_bf16(x), x))


def is_f32(x):
    x = x.to(F64)
    return bool(torch.equal(x.float().double(), x))


# ------------------------------------------------------------------------------------------------------------ layers
def maxpool3x3s2(x, magnitude=False):
    """x [B, H, W, C] -> [B, OH, OW, C]: max over the 3x3 window at stride 2, pad 1 (padding never wins); a window that
    holds a NaN gives NaN (torch's rule: ``val > max || isnan(val)``)."""
    x = x.to(F64)
    if magnitude:
        x = x.abs()
    B, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = torch.full((B, H + 2, W + 2, C), -math.inf, dtype=F64)
    pad[:, 1:H + 1, 1:W + 1] = x
    m = torch.full((B, OH, OW, C), -math.inf, dtype=F64)
    nan = torch.zeros(B, OH, OW, C, dtype=torch.bool)
    for dy in range(3):
        for dx in range(3):
            v = pad[:, dy:dy + 2 * OH - 1:2, dx:dx + 2 * OW - 1:2]
            nan |= v.isnan()
            m = torch.maximum(m, torch.where(v.isnan(), torch.full_like(v, -math.inf), v))
    return torch.where(nan, torch.full_like(m, math.nan), m)


def global_mean(x, channels, magnitude=False):
    """x [B, P, ld] -> [B, channels]: mean over the pixels of the first ``channels`` columns."""
    x = x[..., :channels].to(F64)
    if magnitude:
        x = x.abs()
    return x.sum(1) / x.shape[1]


def dense(x, w, scale=None, bias=None, act=ACT_NONE, magnitude=False):
    """act(scale[n] * sum_k w[n, k] x[b, k] + bias[n]).

    magnitude: the same on absolute values.  relu is 1-Lipschitz, S passes through.  sigmoid has slope <= 1/4 and a
    relative evaluation error of its own, so S = S_linear / 4 + sigmoid(value): with n = n_linear + SIGMOID_ROUNDINGS,
    (n + 2) u S covers (n_linear + 2) u S_linear / 4 (the argument's error through the slope) plus SIGMOID_ROUNDINGS u sigmoid."""
    x, w = x.to(F64), w.to(F64)
    scale = None if scale is None else scale.to(F64)
    bias = None if bias is None else bias.to(F64)

    def lin(x, w, scale, bias):
        v = (x[:, None, :] * w[None, :, :]).sum(-1)
        if scale is not None:
            v = v * scale
        if bias is not None:
            v = v + bias
        return v

    v = lin(x, w, scale, bias)
    if not magnitude:
        return v.clamp_min(0) if act == ACT_RELU else 1 / (1 + torch.exp(-v)) if act == ACT_SIGMOID else v
    S = lin(x.abs(), w.abs(), None if scale is None else scale.abs(), None if bias is None else bias.abs())
    return S / 4 + 1 / (1 + torch.exp(-v)) if act == ACT_SIGMOID else S


def _src(n_out, n_in):
    """bilinear x2, align_corners=False: source coordinate max(0.5 (o + 0.5) - 0.5, 0), its two taps and the weight of the
    second."""
    s = (0.5 * (torch.arange(n_out, dtype=F64) + 0.5) - 0.5).clamp_min(0)
    i0 = s.floor().long()
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0


def bilinear2x(x, magnitude=False):
    """x [B, H, W, C] -> [B, 2H, 2W, C]."""
    x = x.to(F64)
    if magnitude:
        x = x.abs()
    B, H, W, C = x.shape
    h0, h1, lh = _src(2 * H, H)
    w0, w1, lw = _src(2 * W, W)
    lh, lw = lh[None, :, None, None], lw[None, None, :, None]
    top = (1 - lw) * x[:, h0][:, :, w0] + lw * x[:, h0][:, :, w1]
    bot = (1 - lw) * x[:, h1][:, :, w0] + lw * x[:, h1][:, :, w1]
    return (1 - lh) * top + lh * bot


def add_mul_sigmoid(a, b, c, magnitude=False):
    """a + b * sigmoid(c); sigmoid(+-inf) is 1 / 0 exactly."""
    a, b, c = a.to(F64), b.to(F64), c.to(F64)
    s = 1 / (1 + torch.exp(-c))
    return a.abs() + b.abs() * s if magnitude else a + b * s


def bsm_compose(buf, logits, D, ctx, sem, thr, magnitude=False):
    """buf [B, P, ld] (depth [0, D), context [D, D + ctx), room for sem + pad columns), logits [B, P, sem_ld >= sem].
    Returns (the composed buffer, p0): context and softmax(logits[..., :sem]) zeroed where p0 = softmax[0] > thr (thr as the
    float32 the C entry receives), pad columns zero, depth columns untouched."""
    buf, logits = buf.to(F64).clone(), logits[..., :sem].to(F64)
    thr = float(np.float32(thr))
    m = logits.max(-1, keepdim=True).values
    e = torch.exp(logits - m)
    p = e / e.sum(-1, keepdim=True)
    keep = (~(p[..., :1] > thr)).to(F64)
    c = buf[..., D:D + ctx]
    buf[..., D:D + ctx] = (c.abs() if magnitude else c) * keep
    buf[..., D + ctx:D + ctx + sem] = p * keep
    buf[..., D + ctx + sem:] = 0
    if magnitude:
        buf[..., :D] = buf[..., :D].abs()
    return buf, p[..., 0]


def deform_cols(x, off, groups, magnitude=False):
    """DCNv1 sampling (3x3, pad 1, stride 1, one deformable group).  x [B, H, W, C], off [B, H, W, >= 18] (dy, dx per tap)
    -> [B, H, W, groups, 9, C / groups]: bilinear sample at (h - 1 + ky + dy, w - 1 + kx + dx); the sample is zero unless
    -1 < position < size in both axes, and a corner outside the image contributes zero."""
    x, off = x.to(F64), off.to(F64)
    if magnitude:
        x = x.abs()
    B, H, W, C = x.shape
    ys = torch.arange(H, dtype=F64)[None, :, None]
    xs = torch.arange(W, dtype=F64)[None, None, :]
    flat = x.reshape(B, H * W, C)
    taps = []
    for t in range(9):
        hf = ys - 1 + t // 3 + off[..., 2 * t]
        wf = xs - 1 + t % 3 + off[..., 2 * t + 1]
        inside = (hf > -1) & (wf > -1) & (hf < H) & (wf < W)
        h0, w0 = hf.floor(), wf.floor()
        lh, lw = hf - h0, wf - w0
        val = torch.zeros(B, H, W, C, dtype=F64)
        for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            hh, ww = (h0 + dh).long(), (w0 + dw).long()
            ok = inside & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)
            idx = (hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1)).reshape(B, H * W, 1).expand(B, H * W, C)
            val = val + torch.gather(flat, 1, idx).reshape(B, H, W, C) * (wt * ok)[..., None]
        taps.append(torch.where(inside[..., None], val, torch.zeros_like(val)))      # outside: +0, whatever x holds
    col = torch.stack(taps, 3)                                                # [B, H, W, 9, C]
    return col.reshape(B, H, W, 9, groups, C // groups).permute(0, 1, 2, 4, 3, 5).contiguous()


def deform_conv(x, off, weight, groups, magnitude=False):
    """DCNv1 forward: weight [cout, C / groups, 3, 3] -> [B, H, W, cout]."""
    col = deform_cols(x, off, groups, magnitude)                              # [B, H, W, g, 9, cpg]
    w = weight.to(F64)
    if magnitude:
        w = w.abs()
    cout, cpg = w.shape[0], w.shape[1]
    wg = w.reshape(groups, cout // groups, cpg, 9)
    out = torch.einsum("bhwgtc,goct->bhwgo", col, wg)
    return out.reshape(*out.shape[:3], cout)


def head_final_conv(hidden, weights, biases, magnitude=False):
    """hidden [nb, B, H, W, hc]; weights[i] [c_i, hc, 3, 3], biases[i] [c_i] -> [B, sum c_i, H, W]: the 3x3 pad-1
    convolution of each branch on its own hidden map, outputs concatenated in branch order."""
    nb, B, H, W, hc = hidden.shape
    hidden = hidden.to(F64)
    if magnitude:
        hidden = hidden.abs()
    outs = []
    for i in range(nb):
        w, b = weights[i].to(F64), biases[i].to(F64)
        if magnitude:
            w, b = w.abs(), b.abs()
        pad = torch.zeros(B, H + 2, W + 2, hc, dtype=F64)
        pad[:, 1:H + 1, 1:W + 1] = hidden[i]
        o = torch.zeros(B, w.shape[0], H, W, dtype=F64)
        for ky in range(3):
            for kx in range(3):
                o = o + torch.einsum("bhwc,oc->bohw", pad[:, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
        outs.append(o + b[None, :, None, None])
    return torch.cat(outs, 1)


# -------------------------------------------------------------------------------------------------------- generators
def gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def ints(shape, g, lo=-3, hi=3):
    """integer-valued float32 in [lo, hi] (bf16 values as well)"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def randn_bf16(shape, g):
    """normal float32 values that are bf16 values: the same tensor serves a kernel and its bf16 twin"""
    return torch.randn(tuple(shape), generator=g).bfloat16().float()


def nan_windows(x):
    """The NaN / -inf window patterns of tests/test_conv_gpu.py::_nan_windows on an NHWC map of at least 7 x 10 (its last
    pattern sits in row 7 of an 11-row map; here in the last row), on the channels the map has: one NaN in a window, a
    window of NaNs only, an all -inf window, -inf beside values, two NaNs in one window."""
    B, H, W, C = x.shape
    assert H >= 7 and W >= 10
    pats = ((0, 3, slice(5, 6), math.nan), (1, slice(0, 2), slice(0, 2), math.nan), (2, slice(0, 2), slice(0, 2), -math.inf),
            (3, 4, slice(6, 7), -math.inf), (4, min(7, H - 1), slice(8, 10), math.nan))
    for c, hs, ws, v in pats:
        x[:, hs, ws, c % C] = v
    return x


def nan_clipped_corner(x):
    """NaN in the last row and column of an even-sized map: the only window that sees it is clipped on both sides.
    -inf everywhere in channel 1's last window as well (C >= 2)."""
    B, H, W, C = x.shape
    assert H % 2 == 0 and W % 2 == 0
    x[:, H - 1, W - 1, 0] = math.nan
    x[:, max(H - 3, 0):, max(W - 3, 0):, 1] = -math.inf                         # the whole (clipped) last window
    return x


def quarter_offsets(B, H, W, off_ld, g, integer=False):
    """offsets [B, H, W, off_ld] on the quarter-pixel grid in [-3, 3] (integers only if ``integer``); columns past 18 hold
    a large value the kernel must not read as an offset."""
    step = 1 if integer else 4
    off = torch.randint(-3 * step, 3 * step + 1, (B, H, W, off_ld), generator=g).float() / step
    off[..., 18:] = 1000.0
    return off


EDGE_POS = (-1.0, -0.75, -0.25, 0.0)               # and size + these: size-1, size-0.75, size-0.25, size


def pixel_class(h, w, H, W):
    """0 corner, 1 edge, 2 interior"""
    return 2 - int(h in (0, H - 1)) - int(w in (0, W - 1))


def edge_targets(size):
    return sorted({p for p in EDGE_POS} | {size + p for p in EDGE_POS})


def edge_offsets(B, H, W, off_ld):
    """Hand-placed rows: every (image, pixel, tap) gets an offset in [-3, 3] that puts its sample position exactly on one of
    {-1, -0.75, -0.25, 0, H-1, H-0.75, H-0.25, H} in the row axis and on one of the same set for W in the column axis.
    Per pixel class (corner / edge / interior) and axis the targets a tap can reach with |offset| <= 3 are taken in turn;
    the column turn runs at another pace than the row turn, so an outside row meets inside columns and the reverse."""
    off = torch.zeros(B, H, W, off_ld)
    off[..., 18:] = 1000.0
    turn = {}
    for b in range(B):
        for h in range(H):
            for w in range(W):
                cls = pixel_class(h, w, H, W)
                for t in range(9):
                    for axis, base, size in ((0, h - 1 + t // 3, H), (1, w - 1 + t % 3, W)):
                        reach = [p for p in edge_targets(size) if abs(p - base) <= 3]
                        k = turn.get((cls, axis), axis)
                        turn[(cls, axis)] = k + 1 + axis * (k % 3 == 0)
                        off[b, h, w, 2 * t + axis] = reach[k % len(reach)] - base
    return off


def sample_positions(off, H, W):
    """[B, H, W, 9] row and column sample positions (float64) of an offset tensor"""
    ys = torch.arange(H, dtype=F64)[None, :, None, None]
    xs = torch.arange(W, dtype=F64)[None, None, :, None]
    t = torch.arange(9)
    return ys - 1 + (t // 3) + off[..., 0:18:2].double(), xs - 1 + (t % 3) + off[..., 1:18:2].double()


def bsm_case(sem, sem_ld, pad, ctx, pixels, D=5, B=2, thr=0.45):
    """(buf [B, pixels, ld] with NaN in the pad columns, logits [B, pixels, sem_ld] with NaN past sem, D, ctx, sem, thr).
    Logits are multiples of 2^-10 below 16 in magnitude, so logit - max is exact in f32 and the bound need not carry it."""
    g = gen(sem, sem_ld, pad, ctx, pixels, 77)
    ld = D + ctx + sem + pad
    buf = torch.randn(B, pixels, ld, generator=g)
    buf[..., D + ctx + sem:] = math.nan
    buf[..., D + ctx:D + ctx + sem] = math.nan      # the semantic columns are written, never read
    logits = (torch.randn(B, pixels, sem_ld, generator=g) * 3).clamp(-15, 15).mul(1024).round().div(1024)
    logits[..., sem:] = math.nan
    return buf, logits, D, ctx, sem, thr


BSM_CASES = [(sem, sem + dl, pad, ctx, px) for sem in (2, 7) for dl in (0, 5) for pad in (0, 1, 9) for ctx in (1, 80)
             for px in (1, 9)]
BSM_EXCLUDE = 1e-6                                  # pixels whose float64 p0 is this close to thr are not judged


def head_case(H, W, hc, widths, B, exact, g):
    """(hidden [nb, B, H, W, hc], weights [c_i, hc, 3, 3] per branch, biases per branch)"""
    nb = len(widths)
    if exact:
        hidden = ints((nb, B, H, W, hc), g)
        ws = [ints((c, hc, 3, 3), g, -2, 2) for c in widths]
        bs = [ints((c,), g) for c in widths]
    else:
        hidden = torch.randn(nb, B, H, W, hc, generator=g)
        ws = [torch.randn(c, hc, 3, 3, generator=g) / (9 * hc) ** 0.5 for c in widths]
        bs = [torch.randn(c, generator=g) for c in widths]
    return hidden, ws, bs
