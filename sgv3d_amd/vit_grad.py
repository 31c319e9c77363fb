"""The adjoints of the SAM ViT encoder's own kernels (csrc/vit_grad.hip) as thin calls and ``torch.autograd.Function``s:
attention with windows, padding tokens and the decomposed relative position, LayerNorm, the exact GELU and the crop + bilinear
resize.  f32 NHWC tensors on the device; linear layers and convolutions take their gradients from ``conv_grad``.

The bf16 training mode (``hip_ops.VIT_TRAIN_BF16``) hands ``attention`` and ``gelu`` bf16 tensors and asks ``layer_norm`` for a bf16
result: the same functions dispatch on the dtype to the bf16 entries (csrc/vit_grad_bf16.hip, sgv3d_layernorm_backward_bf16dy,
sgv3d_gelu_backward_bf16).  Parameters and their gradients stay f32.

Under ``torch.no_grad()``, or when no input requires grad, the Functions run the forward entries alone: no lse is written and no
backward entry is ever launched.  There is no CPU fallback: every function raises if the HIP library is missing.
"""
import ctypes

import torch

from . import _lib

__all__ = ['attention', 'layer_norm', 'gelu', 'resize_bilinear', 'attention_lse', 'attention_backward', 'layernorm_backward',
           'gelu_backward', 'resize_bilinear_backward']


def _f32(*tensors):
    for t in tensors:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "contiguous float32 tensors on the GPU are expected"


def _bf16(*tensors):
    for t in tensors:
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous(), "contiguous bfloat16 tensors on the GPU are expected"


# ---- thin calls ----
def attention_lse(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None):
    """sgv3d_vit_attention_lse: -> out [B, H, W, C] (the bits of sgv3d_vit_attention), lse [B, heads, H, W].  A bf16 ``qkv``:
    sgv3d_vit_attention_bf16_lse, a bf16 ``out`` (the bits of sgv3d_vit_attention_bf16) and the f32 lse."""
    t16 = qkv.dtype == torch.bfloat16
    _bf16(qkv) if t16 else _f32(qkv)
    _f32(pad_qkv, rel_pos_h, rel_pos_w)
    name = "sgv3d_vit_attention_bf16_lse" if t16 else "sgv3d_vit_attention_lse"
    d = _lib.vit_attn_desc(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w)
    out = torch.empty(d.batch, d.height, d.width, d.heads * d.head_dim, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(d.batch, d.heads, d.height, d.width, dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = getattr(_lib.load(), name)(ctypes.byref(d), qkv.data_ptr(), _lib.ptr(pad_qkv), _lib.ptr(rel_pos_h), _lib.ptr(rel_pos_w),
                                        out.data_ptr(), lse.data_ptr(), _lib.stream_handle(qkv.device))
    _lib.check(rc, name)
    return out, lse


def attention_backward(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w, out, lse, dout):
    """sgv3d_vit_attention_backward: -> dqkv, dpad_qkv (None without pad_qkv), drel_pos_h, drel_pos_w (None without tables).
    bf16 ``qkv``, ``out`` and ``dout``: sgv3d_vit_attention_bf16_backward, a bf16 ``dqkv`` and f32 parameter gradients."""
    t16 = qkv.dtype == torch.bfloat16
    _bf16(qkv, out, dout) if t16 else _f32(qkv, out, dout)
    _f32(pad_qkv, rel_pos_h, rel_pos_w, lse)
    name = "sgv3d_vit_attention_bf16_backward" if t16 else "sgv3d_vit_attention_backward"
    d = _lib.vit_attn_desc(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w)
    assert out.shape == dout.shape == (d.batch, d.height, d.width, d.heads * d.head_dim) and lse.shape == (d.batch, d.heads, d.height, d.width)
    dev = qkv.device
    lib = _lib.load()
    dqkv = torch.empty_like(qkv)
    dpad = None if pad_qkv is None else torch.empty_like(pad_qkv)
    drh = None if rel_pos_h is None else torch.empty_like(rel_pos_h)
    drw = None if rel_pos_w is None else torch.empty_like(rel_pos_w)
    nws = int(getattr(lib, name + "_workspace_bytes")(ctypes.byref(d)))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(ctypes.byref(d), qkv.data_ptr(), _lib.ptr(pad_qkv), _lib.ptr(rel_pos_h), _lib.ptr(rel_pos_w),
                                out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), _lib.ptr(dpad),
                                _lib.ptr(drh), _lib.ptr(drw), ws.data_ptr(), nws, _lib.stream_handle(dev))
    _lib.check(rc, name)
    return dqkv, dpad, drh, drw


def layernorm_backward(x, weight, eps, dy):
    """sgv3d_layernorm_backward over the last dimension: -> dx, dweight, dbias (f32).  A bf16 ``dy`` (the gradient of a bf16 result):
    sgv3d_layernorm_backward_bf16dy, the same arithmetic on the widened dy."""
    t16 = dy.dtype == torch.bfloat16
    _f32(x, weight)
    _bf16(dy) if t16 else _f32(dy)
    name = "sgv3d_layernorm_backward_bf16dy" if t16 else "sgv3d_layernorm_backward"
    c = int(x.shape[-1])
    rows = x.numel() // c
    assert dy.shape == x.shape and weight.numel() == c
    lib = _lib.load()
    dx, dw, db = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(weight)
    nws = int(lib.sgv3d_layernorm_backward_workspace_bytes(rows, c))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = getattr(lib, name)(rows, c, x.data_ptr(), weight.data_ptr(), float(eps), dy.data_ptr(), dx.data_ptr(),
                                dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nws, _lib.stream_handle(x.device))
    _lib.check(rc, name)
    return dx, dw, db


def gelu_backward(x, dy):
    """sgv3d_gelu_backward: dy (Phi(x) + x phi(x)), ``x`` the pre-activation.  bf16 ``x`` and ``dy``: sgv3d_gelu_backward_bf16."""
    t16 = x.dtype == torch.bfloat16
    _bf16(x, dy) if t16 else _f32(x, dy)
    name = "sgv3d_gelu_backward_bf16" if t16 else "sgv3d_gelu_backward"
    assert x.shape == dy.shape
    dx = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), name)(x.numel(), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), _lib.stream_handle(x.device))
    _lib.check(rc, name)
    return dx


def resize_bilinear_backward(dy, in_hw, crop):
    """sgv3d_resize_bilinear_backward: dy NHWC [B, oh, ow, C] -> dx [B, h, w, C], zero outside the crop."""
    _f32(dy)
    b, oh, ow, c = (int(s) for s in dy.shape)
    dx = torch.empty(b, int(in_hw[0]), int(in_hw[1]), c, dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        rc = _lib.load().sgv3d_resize_bilinear_backward(b, int(in_hw[0]), int(in_hw[1]), c, int(crop[0]), int(crop[1]), oh, ow,
                                                        dy.data_ptr(), dx.data_ptr(), _lib.stream_handle(dy.device))
    _lib.check(rc, "sgv3d_resize_bilinear_backward")
    return dx


def _differentiating(*tensors):
    """Whether autograd will ask for a gradient: grad mode on and an input that requires grad.  Otherwise the Functions below are
    not entered at all: the forward entries alone run, nothing is saved and no lse is written."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _gelu_forward(x):
    name = "sgv3d_gelu_bf16" if x.dtype == torch.bfloat16 else "sgv3d_gelu"
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), name)(x.numel(), x.data_ptr(), y.data_ptr(), _lib.stream_handle(x.device))
    _lib.check(rc, name)
    return y


def _forward_ops():
    from .layers.backbones import common, sam_encoder       # (these import this package's hip_ops: not at module level)
    return common, sam_encoder


# ---- autograd ----
class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, pad_qkv, rel_pos_h, rel_pos_w, num_heads, window):
        ctx.geom = (int(num_heads), (int(window[0]), int(window[1])))
        out, lse = attention_lse(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w)
        ctx.save_for_backward(qkv, pad_qkv, rel_pos_h, rel_pos_w, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, pad_qkv, rel_pos_h, rel_pos_w, out, lse = ctx.saved_tensors
        dqkv, dpad, drh, drw = attention_backward(qkv, ctx.geom[0], ctx.geom[1], pad_qkv, rel_pos_h, rel_pos_w, out, lse, dout.contiguous())
        return dqkv, dpad, drh, drw, None, None


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype=None):
        ctx.eps = float(eps)
        ctx.save_for_backward(x, weight)
        return _forward_ops()[0].layernorm(x, weight, bias, eps, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dw, db = layernorm_backward(x, weight, ctx.eps, dy.contiguous())
        return dx, dw, db, None, None


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _gelu_forward(x)

    @staticmethod
    def backward(ctx, dy):
        return gelu_backward(ctx.saved_tensors[0], dy.contiguous())


class _ResizeBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, crop, size):
        ctx.geom = ((int(x.shape[1]), int(x.shape[2])), (int(crop[0]), int(crop[1])))
        return _forward_ops()[1].resize_bilinear(x, crop, size)

    @staticmethod
    def backward(ctx, dy):
        return resize_bilinear_backward(dy.contiguous(), *ctx.geom), None, None


def attention(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None):
    """``sam_encoder.vit_attention``, differentiable in ``qkv``, ``pad_qkv`` and both tables.  Saves qkv, out and lse [B, heads, H, W];
    the backward recomputes P tile by tile.  ``pad_qkv``'s gradient has an exactly zero q part.  A bf16 ``qkv``: the bf16 entries
    (``sam_encoder.vit_attention_bf16`` and its adjoint); out and the saved tensors are bf16, the parameters stay f32."""
    t16 = qkv.dtype == torch.bfloat16
    _bf16(qkv) if t16 else _f32(qkv)
    _f32(pad_qkv, rel_pos_h, rel_pos_w)
    if not _differentiating(qkv, pad_qkv, rel_pos_h, rel_pos_w):
        attend = _forward_ops()[1].vit_attention_bf16 if t16 else _forward_ops()[1].vit_attention
        return attend(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w)
    return _Attention.apply(qkv, pad_qkv, rel_pos_h, rel_pos_w, num_heads, window)


def layer_norm(x, weight, bias, eps, out_dtype=None):
    """LayerNorm over the last dimension (``nn.LayerNorm`` and ``LayerNorm2d`` on NHWC), differentiable; saves ``x`` alone (mean and
    rstd are recomputed).  ``out_dtype=torch.bfloat16``: the bf16 result of sgv3d_layernorm_bf16out, whose gradient arrives as bf16."""
    _f32(x, weight, bias)
    if not _differentiating(x, weight, bias):
        return _forward_ops()[0].layernorm(x, weight, bias, eps, out_dtype=out_dtype)
    if out_dtype is None:
        return _LayerNorm.apply(x, weight, bias, eps)
    return _LayerNorm.apply(x, weight, bias, eps, out_dtype)


def gelu(x):
    """Exact GELU, out of place: the pre-activation is what the backward reads.  f32 or bf16."""
    _bf16(x) if x.dtype == torch.bfloat16 else _f32(x)
    return _Gelu.apply(x) if _differentiating(x) else _gelu_forward(x)


def resize_bilinear(x, crop, size):
    """``sam_encoder.resize_bilinear`` (NHWC crop + bilinear resize), differentiable in ``x``."""
    _f32(x)
    if not _differentiating(x):
        return _forward_ops()[1].resize_bilinear(x, crop, size)
    return _ResizeBilinear.apply(x, crop, size)
