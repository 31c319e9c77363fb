"""The float64 attention forward and backward of tests/vit_grad_ref.py with the rounding points of the bf16 kernels
(csrc/vit_bf16.hip, csrc/vit_grad_bf16.hip) switchable.  With every switch off it IS tests/vit_grad_ref.py's arithmetic (checked
to 1e-12 in tests/test_vit_grad_bf16_cpu.py); with them on it rounds where the kernels round:

  operands   q, k, v and dO are bf16 values (the tensors are; the f32 pad_qkv and tables are rounded to bf16 on the way in)
  p_ds       forward: P = exp(s - m) rounded to bf16, l the sum of the ROUNDED P, O / l rounded to bf16, lse = m + log l;
             backward: P = exp(s - lse) and dS = P (dP - delta) rounded to bf16 once as the operands of dV, dK and dQ;
             A_h, A_w (the table gradients and the table terms of dq) use the unrounded dS, as the kernel's f32 sums do
  f32_sums   every product-and-sum (the logits, P V, dP, delta, dV, dK, dQ, A_h, A_w, the table and padding gradients), the
             exponentials and lse run in float32 arithmetic, as the kernels' f32 accumulators do: sums that agree exactly in
             float64 (dP and delta of a one-key window) then differ by their summation orders, as they do in any f32 kernel
  dqkv is rounded to bf16 once (``operands``): it is a bf16 tensor.

The tests' bar for a kernel output is 4 x the error of the all-on run against the all-off run on the same inputs.
"""
import torch

import vit_ref as V
from vit_grad_ref import _windows


def bf16(t):
    """Round to the nearest bf16 value (ties to even), keep the dtype."""
    return t.float().bfloat16().to(t.dtype)


class _Arith:
    """The arithmetic of the sums: float64 as it stands, or float32 (``f32_sums``) with float64 tensors in and out."""

    def __init__(self, f32):
        self.f32 = f32

    def __call__(self, fn, *tensors):
        if not self.f32:
            return fn(*tensors)
        return fn(*(None if t is None else t.float() for t in tensors)).double()


def _prepare(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w, operands):
    r = (lambda t: None if t is None else bf16(t)) if operands else (lambda t: t)
    qkv, pad_qkv, rel_pos_h, rel_pos_w = r(qkv), r(pad_qkv), r(rel_pos_h), r(rel_pos_w)
    q, k, v, real = V.split_windows(qkv, num_heads, window, pad_qkv)
    return q, k, v, real, rel_pos_h, rel_pos_w


def _forward(q, k, v, window, rh, rw, p_ds, f32_sums):
    ar = _Arith(f32_sums)
    s = ar(lambda q, k, rh, rw: V.window_logits(q, k, window, rh, rw), q, k, rh, rw)
    if not p_ds:
        lse = ar(lambda s: torch.logsumexp(s, -1, keepdim=True), s)
        return s, lse, ar(lambda s, lse, v: torch.exp(s - lse) @ v, s, lse, v)
    m = s.max(-1, keepdim=True).values
    p = bf16(ar(lambda s, m: torch.exp(s - m), s, m))
    l = ar(lambda p: p.sum(-1, keepdim=True), p)
    return s, ar(lambda m, l: m + torch.log(l), m, l), bf16(ar(lambda p, v, l: (p @ v) / l, p, v, l))


def attention_forward(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None, operands=False, p_ds=False, f32_sums=False):
    """-> out [B, H, W, C], lse [B, heads, H, W] (natural-log units)."""
    b, h, w, _ = qkv.shape
    q, k, v, _, rh, rw = _prepare(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w, operands)
    _, lse, o = _forward(q, k, v, window, rh, rw, p_ds, f32_sums)
    return V.merge_windows(o, window, h, w), V.merge_windows(lse, window, h, w).permute(0, 3, 1, 2).contiguous()


def attention_backward(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w, dout, operands=False, p_ds=False, f32_sums=False):
    """-> dqkv [B, H, W, 3 C], dpad_qkv [3 C], drel_pos_h, drel_pos_w (None without tables)."""
    b, h, w, c3 = qkv.shape
    wh, ww = window
    hd = c3 // 3 // num_heads
    scale = hd ** -0.5
    q, k, v, real, rh_t, rw_t = _prepare(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w, operands)
    s, lse, o = _forward(q, k, v, window, rh_t, rw_t, p_ds, f32_sums)
    ar = _Arith(f32_sums)
    do = _windows(bf16(dout) if operands else dout, num_heads, window)      # zero rows for the padding slots: never a query
    delta = ar(lambda do, o: (do * o).sum(-1, keepdim=True), do, o)
    dp = ar(lambda do, v: do @ v.transpose(-1, -2), do, v)
    # a padding slot is never a query: its row of P is not part of the function
    qreal = real.to(qkv.dtype)[None, :, :, None, :, None]
    p = ar(lambda s, lse: torch.exp(s - lse), s, lse) * qreal
    ds = ar(lambda p, dp, delta: p * (dp - delta), p, dp, delta)
    p_op, ds_op = (bf16(p), bf16(ds)) if p_ds else (p, ds)
    dv = ar(lambda p, do: p.transpose(-1, -2) @ do, p_op, do)
    dk = ar(lambda ds, q: scale * (ds.transpose(-1, -2) @ q), ds_op, q)
    dq = ar(lambda ds, k: scale * (ds @ k), ds_op, k)
    drh = drw = None
    if rel_pos_h is not None:
        lead = ds.shape[:-2]
        ih, iw = torch.arange(wh), torch.arange(ww)
        idx_h = ih[:, None] - ih[None, :] + wh - 1
        idx_w = iw[:, None] - iw[None, :] + ww - 1
        a_h = ar(lambda ds: ds.reshape(*lead, wh, ww, wh, ww).sum(-1), ds)
        a_w = ar(lambda ds: ds.reshape(*lead, wh, ww, wh, ww).sum(-2), ds)
        rh, rw = rh_t.to(qkv.dtype)[idx_h], rw_t.to(qkv.dtype)[idx_w]
        dq = ar(lambda dq, a_h, a_w, rh, rw: dq + (torch.einsum('...hwa,had->...hwd', a_h, rh)
                                                  + torch.einsum('...hwb,wbd->...hwd', a_w, rw)).reshape(dq.shape), dq, a_h, a_w, rh, rw)
        n = a_h.numel() // (wh * ww * wh)

        def tables(a_h, a_w, q):
            qq = q.reshape(n, wh, ww, hd)
            gh = torch.einsum('nhwa,nhwd->had', a_h.reshape(n, wh, ww, wh), qq)
            gw = torch.einsum('nhwb,nhwd->wbd', a_w.reshape(n, wh, ww, ww), qq)
            return torch.cat([torch.zeros(2 * wh - 1, hd, dtype=q.dtype).index_add_(0, idx_h.reshape(-1), gh.reshape(-1, hd)),
                              torch.zeros(2 * ww - 1, hd, dtype=q.dtype).index_add_(0, idx_w.reshape(-1), gw.reshape(-1, hd))])
        both = ar(tables, a_h, a_w, q)
        drh, drw = both[:2 * wh - 1], both[2 * wh - 1:]
    dqkv = torch.cat([V.merge_windows(t, window, h, w) for t in (dq, dk, dv)], -1)
    if operands:
        dqkv = bf16(dqkv)
    m = (~real).to(qkv.dtype)[None, :, :, None, :, None]
    dpad = ar(lambda dk, dv, m: torch.stack([torch.zeros_like(dk[0, 0, 0, :, 0]), (dk * m).sum((0, 1, 2, 4)), (dv * m).sum((0, 1, 2, 4))]), dk, dv, m)
    return dqkv, dpad.reshape(-1), drh, drw


ALL_ON = dict(operands=True, p_ds=True, f32_sums=True)
