"""Shared pieces of the convolution-geometry tests (test_conv_geometry_cpu.py, test_conv_geometry_gpu.py); imports without a GPU.

Dyadic data.  Activations, upstream gradients and residuals are k / 4 with |k| <= 8, weights k / 4 with |k| <= 4, epilogue scales come
from {0.5, 1, 2} and shifts are multiples of 1 / 4.  Every product of an activation (or gradient) and a weight is a multiple of 1 / 16
of magnitude at most 2, so a sum of K <= 2304 of them is a multiple of 1 / 16 below 2^13: exact in f32 whatever the order of the
additions (24 bits cover 2^13 * 16 = 2^17), still exact after a scale of 0.5 .. 2 and a shift / residual of a few units.  Every
operand has at most 4 significant bits: exact in bf16, and an f32x3 split of it has only its hi term.  The float64 reference is
therefore the EXACT expected output of the f32, f32x3 and bf16 kernels alike (a bf16 output: that value rounded once), and every
comparison of these tests is ``torch.equal``.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

K_MAX = 2304                    # products per output element for which ``assert_exact`` vouches

# One PackedConv layer: [cout, cin, kh, kw] weights at stride / pad / dil on a [B, H, W, cin] map.  ``kind`` (dgrad_forms):
# 'rot' = the 180-degree-rotated layer, 'phase' = one parity of the stride-2 decomposition, 'patchify' = the transposed convolution
Form = namedtuple("Form", "cin cout kh kw stride pad dil H W kind", defaults=("",))


def out_hw(H, W, kh, kw, stride, pad, dil):
    return (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1


def assert_exact(terms, max_product=2.0, unit=1.0 / 16):
    """A sum of ``terms`` products, each a multiple of ``unit`` of magnitude <= ``max_product``, scaled by at most 2 and moved by a
    shift and a residual (|.| <= 4, multiples of 1 / 4) is an f32 value, and so is every partial sum in any order."""
    assert terms <= K_MAX, f"{terms} products per output: the dyadic data only vouches for {K_MAX}"
    assert (2.0 * terms * max_product + 8.0) / (unit / 2) < 2.0 ** 24


def dyadic(shape, bound, gen):
    """k / 4 with |k| <= bound, f32."""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen).float() / 4


def epilogue(cout, gen):
    """(scale, shift) of the fused epilogue: scales from {0.5, 1, 2}, shifts multiples of 1 / 4 (|.| <= 2)."""
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=gen)]
    return scale, dyadic((cout,), 8, gen)


def conv_ref(x, w, stride=1, pad=0, dil=1, scale=None, shift=None, residual=None, relu=False):
    """float64 ``act(conv2d(x, w) * scale + shift + residual)`` for NHWC ``x`` and OIHW ``w`` (any kh x kw)."""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, stride, pad, dil).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale.double() + shift.double()
    if residual is not None:
        y = y + residual.double()
    return (y.clamp_min(0) if relu else y).contiguous()


def assert_discriminates(x, w, stride, pad, dil):
    """The data can tell tap orders apart: the reference of ``w`` is not the reference of ``w`` flipped along an axis that has more
    than one tap (``w.flip(2)``, ``w.flip(3)``), of ``w.transpose(2, 3)`` (where that output has the same shape at all), nor of ``w``
    with its taps decoded by the other axis' length (``tap // kh`` for ``tap // kw``: the mix-up that keeps every shape)."""
    cout, cin, kh, kw = w.shape
    ref = conv_ref(x, w, stride, pad, dil)
    assert float(ref.abs().max()) > 0
    for axis in (2, 3):
        if w.shape[axis] > 1:
            assert not torch.equal(ref, conv_ref(x, w.flip(axis), stride, pad, dil)), f"flip({axis}) goes unnoticed"
    if kh != kw:
        oh, ow = out_hw(x.shape[1], x.shape[2], kw, kh, stride, pad, dil)
        if oh > 0 and ow > 0:
            other = conv_ref(x, w.transpose(2, 3), stride, pad, dil)
            assert other.shape != ref.shape or not torch.equal(ref, other), "transpose(2, 3) goes unnoticed"
        if kh > 1 and kw > 1:
            mixed = w.reshape(cout, cin, kw, kh).transpose(2, 3)
            assert not torch.equal(ref, conv_ref(x, mixed, stride, pad, dil)), "a kh / kw mix-up of the tap decode goes unnoticed"
    return ref


# ------------------------------------------------------------------------------------------- conv2d_backward_data's decomposition
def _need(P, T, n_in, n_out):
    """conv_grad._dgrad_stride2's ``need``: the symmetric padding that covers the low side and yields n_out outputs."""
    return max(P, 0, n_out - n_in + T - 1 - P)


def stride2_phases(k, pad, H, W):
    """The four phases of ``conv_grad._dgrad_stride2`` for a k x k / stride 2 / ``pad`` layer on an H x W input, (py, px) in its order:
    None for a phase without taps or pixels, else dict(ty, tx: tap indices in correlation order; p_y, p_x: low padding; n_y, n_x:
    pixels of the phase; pp: the one symmetric padding of the sub-convolution; oh, ow: the sub-convolution's output; hc, wc: dY)."""
    from sgv3d_amd.conv_grad import _phase_1d
    hc, wc = out_hw(H, W, k, k, 2, pad, 1)
    phases = []
    for py in range(2):
        ty, p_y, n_y = _phase_1d(k, pad, py, hc, H)
        for px in range(2):
            tx, p_x, n_x = _phase_1d(k, pad, px, wc, W)
            if not ty or not tx or n_y == 0 or n_x == 0:
                phases.append(None)
                continue
            pp = max(_need(p_y, len(ty), hc, n_y), _need(p_x, len(tx), wc, n_x))
            phases.append(dict(ty=ty, tx=tx, p_y=p_y, p_x=p_x, n_y=n_y, n_x=n_x, pp=pp, hc=hc, wc=wc,
                               oh=hc + 2 * pp - (len(ty) - 1), ow=wc + 2 * pp - (len(tx) - 1)))
    return phases


def dgrad_forms(k, stride, pad, dil, H, W, cin, cout):
    """The PackedConv layers ``conv_grad.conv2d_backward_data`` builds for the data gradient of a k x k convolution cin -> cout at
    stride / pad / dil on an H x W input -- in the layer's own terms: it reads dY's ``cout`` channels padded to 4 and writes ``cin``."""
    cp = (cout + 3) // 4 * 4
    hc, wc = out_hw(H, W, k, k, stride, pad, dil)
    assert hc > 0 and wc > 0
    if k == stride and stride > 1 and pad == 0 and dil == 1:
        return [Form(cp, cin, k, k, stride, 0, 1, hc, wc, "patchify")]
    rpad = dil * (k - 1) - pad
    if stride == 1 or (k == 1 and pad == 0):
        assert rpad >= 0
        return [Form(cp, cin, k, k, 1, rpad, dil, hc, wc, "rot")]
    if stride == 2 and dil == 1:
        return [Form(cp, cin, len(p["ty"]), len(p["tx"]), 1, p["pp"], 1, hc, wc, "phase") for p in stride2_phases(k, pad, H, W) if p]
    assert rpad >= 0
    return [Form(cp, cin, k, k, 1, rpad, dil, H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1), "rot")]


def dgrad_stride2_reference(dy, w, in_hw, pad, conv=None):
    """``conv_grad._dgrad_stride2`` restated on the CPU: the four sub-convolutions through ``conv`` (default: float64 F.conv2d), the
    interleave by slicing -- under the cover condition sgv3d_interleave_phases2 enforces.  NHWC ``dy``, OIHW ``w``; returns NHWC dX."""
    conv = conv or (lambda x, sub, pp: conv_ref(x, sub, 1, pp, 1))
    cout, cin, k, _ = w.shape
    H, W = in_hw
    dx = torch.zeros(dy.shape[0], H, W, cin, dtype=torch.float64)
    for i, p in enumerate(stride2_phases(k, pad, H, W)):
        py, px = i >> 1, i & 1
        need_h, need_w = (H - py + 1) // 2, (W - px + 1) // 2          # the launcher's count of this phase's pixels
        if p is None:
            continue                                                   # a zero phase of max(n, 1) pixels at offset 0: covers by construction
        assert (p["hc"], p["wc"]) == tuple(dy.shape[1:3]) and (need_h, need_w) == (p["n_y"], p["n_x"])
        sub = w[:, :, min(p["ty"])::2, min(p["tx"])::2].flip(2, 3).transpose(0, 1).contiguous()
        assert tuple(sub.shape[2:]) == (len(p["ty"]), len(p["tx"]))
        o = conv(dy, sub, p["pp"])
        row0, col0 = p["pp"] - p["p_y"], p["pp"] - p["p_x"]
        assert tuple(o.shape[1:3]) == (p["oh"], p["ow"])
        assert row0 >= 0 and col0 >= 0 and row0 + need_h <= o.shape[1] and col0 + need_w <= o.shape[2], "phase does not cover its pixels"
        dx[:, py::2, px::2] = o[:, row0:row0 + need_h, col0:col0 + need_w].double()
    return dx


def autograd_reference(x, w, dy, stride, pad, dil):
    """float64 (y, dx, dw) of ``y = conv2d(x, w)`` under the upstream gradient ``dy``; NHWC activations, OIHW weights."""
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr = w.double().clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride, pad, dil)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), xr.grad.permute(0, 2, 3, 1).contiguous(), wr.grad
