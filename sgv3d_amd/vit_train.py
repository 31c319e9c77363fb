"""Training forward of SAM's ViT image encoder (layers/backbones/sam_encoder.py), differentiable in every parameter.

The modules' own ``forward`` / ``embed`` stay inference only.  Training is opt-in through these functions, which read the same
modules' parameters and give the same values:

  attention_forward(attn, x, window, residual)   Attention.forward
  block_forward(blk, x)                          Block.forward
  encoder_forward(enc, x)                        ImageEncoderViT.forward  (the [B, out_chans, h, w] permuted view)
  encoder_embed(enc, x)                          ImageEncoderViT.embed    (the NHWC neck output)

* every linear layer (its weight viewed as [out, in, 1, 1]), the neck's 1x1 and 3x3 and the patch embedding (kernel == stride;
  weight and bias gradients only: the image gets none) run the module's own ``PackedConv`` forward -- the same packed weights,
  tile choice and fused residual add as the inference path, which is what makes the outputs bit-equal -- and take their data and
  weight gradients from ``conv_grad.conv2d_backward_data`` / ``conv2d_backward_weight``;
* attention, LayerNorm, GELU and the crop + resize are the autograd Functions of ``vit_grad`` (csrc/vit_grad.hip);
* ``pos_embed`` and the two shortcuts of a block are added in the epilogues of the patch embedding, proj and lin2, as in the
  inference path; their gradient is the upstream gradient;
* ``attn.qkv.bias`` is also q, k, v of the tokens the window padding adds, so its gradient is the linear layer's bias gradient
  plus the attention's ``dpad_qkv``: autograd adds the two because the same parameter feeds both.

Training runs the f32-tensor path whatever ``hip_ops.VIT_BF16`` says.  Its own switch is ``hip_ops.VIT_TRAIN_BF16``: on a Block
for which ``hip_ops.vit_train_bf16_active`` holds, ``block_forward`` runs the launches of ``Block.forward`` in bf16 mode
(sgv3d_layernorm_bf16out, qkv bf16 -> bf16, sgv3d_vit_attention_bf16, proj bf16 -> f32 + shortcut, sgv3d_layernorm_bf16out, lin1
bf16 -> bf16, sgv3d_gelu_bf16, lin2 bf16 -> f32 + shortcut), bit-equal to that module forward, saves the bf16 tensors themselves and
runs their adjoints on bf16 tensors (csrc/vit_grad_bf16.hip, ``conv_grad`` on bf16 maps).  The residual stream, the patch
embedding, ``pos_embed`` and the neck keep f32 tensors; every parameter gradient is f32.  Off, or on a Block that is not covered:
the f32-tensor path, every call and every bit as without the switch.

There is no CPU path; an image that requires grad, a CPU tensor and a shape outside ``hip_ops.vit_train_covers`` raise before any
launch.
"""
import torch

from . import _lib, conv_grad, hip_ops, vit_grad
from .layers.backbones.sam_encoder import _norm_params

__all__ = ['attention_forward', 'block_forward', 'encoder_forward', 'encoder_embed']


def _require(x, what, image=False, bf16_ok=False):
    if not isinstance(x, torch.Tensor):
        raise _lib.SGV3DError(f"{what}: a tensor is expected")
    if image and x.requires_grad:
        raise _lib.SGV3DError(f"{what}: the image x requires grad, and there is no gradient with respect to the image")
    if not x.is_cuda:
        raise _lib.SGV3DError(f"{what}: the input must be a tensor on the GPU (there is no CPU fallback)")
    if x.dtype != torch.float32 and not (bf16_ok and x.dtype == torch.bfloat16):
        raise _lib.SGV3DError(f"{what}: float32 input expected, got {x.dtype}")
    _lib.load()


def _covers(dim, num_heads, what):
    if not hip_ops.vit_train_covers(dim, num_heads):
        raise _lib.SGV3DError(f"{what}: dim {dim} with {num_heads} heads is outside hip_ops.vit_train_covers "
                              "(head_dim 32, 64 or 80, dim a multiple of 4)")


class _PackedLayer(torch.autograd.Function):
    """One linear layer or convolution of the encoder: the forward is the module's own ``PackedConv`` call (the same packed weights,
    tile choice and fused ``residual`` add as the inference path, hence the same bits); the backward is ``conv_grad``'s data- and
    weight-gradient kernels, the bias gradient a sum over the pixels, and the residual's gradient the upstream gradient itself.

    The bf16 mode's io pairs: bf16 in, bf16 out (qkv, lin1: ``out_dtype`` bf16) and bf16 in, f32 out (proj, lin2).  ``conv_grad``
    takes ``x`` and ``dy`` of one dtype, so the f32 ``dy`` of the mixed pair is rounded to bf16 once and that copy feeds both
    gradients (in bf16 compute mode the gradient kernels round their operands to bf16 while staging: the same operand bits either
    way); the residual branch passes the f32 ``dy`` through, and the bias gradient sums the upstream gradient in f32.  ``dx`` is bf16."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, packed, kw, out_dtype=None):
        ctx.save_for_backward(x, weight)
        ctx.geom = (int(kw.get('stride', 1)), int(kw.get('pad', 0)))
        if out_dtype is None:
            return packed.get(weight, bias, **kw)(x, residual=residual)
        return packed.get(weight, bias, **kw)(x, residual=residual, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        stride, pad = ctx.geom
        dy = dy.contiguous()
        w4 = weight.detach().reshape(weight.shape[0], weight.shape[1], 1, 1) if weight.dim() == 2 else weight.detach()
        cout, cin, kh, kw = (int(v) for v in w4.shape)
        dx = dw = db = None
        # bf16 mode: the operand of both gradient kernels is dy as bf16 (the mixed pair's f32 dy rounded once)
        dyx = dy.to(torch.bfloat16) if x.dtype == torch.bfloat16 and dy.dtype != torch.bfloat16 else dy
        if ctx.needs_input_grad[0]:
            dx = conv_grad.conv2d_backward_data(dyx, w4, (int(x.shape[1]), int(x.shape[2])), stride, pad)
        if ctx.needs_input_grad[1]:
            dw = conv_grad.conv2d_backward_weight(x, dyx, (kh, kw), stride, pad, cin=cin, cout=cout).reshape(weight.shape)
        if ctx.needs_input_grad[2]:
            db = dy.sum((0, 1, 2), dtype=torch.float32) if dy.dtype == torch.bfloat16 else dy.sum((0, 1, 2))
        return dx, dw, db, (dy if ctx.needs_input_grad[3] else None), None, None, None


def _packed(packed, x, weight, bias=None, residual=None, out_dtype=None, **kw):
    """``kw``: what the module itself hands to ``PackedParam.get`` for this layer.  ``out_dtype``: bf16 for the bf16 -> bf16 layers
    of the bf16 mode (None: the layer's f32 result)."""
    if out_dtype is None:
        return _PackedLayer.apply(x, weight, bias, residual, packed, kw)
    return _PackedLayer.apply(x, weight, bias, residual, packed, kw, out_dtype)


def attention_forward(attn, x, window=None, residual=None):
    """``Attention.forward`` of ``attn`` on the normed, un-partitioned map x [B, H, W, C]; ``residual`` is added to the result.  A bf16
    ``x`` (what ``block_forward`` hands over in the bf16 mode): qkv and the attention output are bf16, proj writes f32."""
    _require(x, "vit_train.attention_forward", bf16_ok=True)
    _covers(attn.qkv.in_features, attn.num_heads, "vit_train.attention_forward")
    _, h, w, _ = x.shape
    window = window or (int(h), int(w))
    rel = (attn.rel_pos_h, attn.rel_pos_w) if attn.use_rel_pos else (None, None)
    if attn.use_rel_pos:
        for name, tab, win in (("rel_pos_h", rel[0], window[0]), ("rel_pos_w", rel[1], window[1])):
            if tab.shape[0] != 2 * win - 1:
                raise _lib.SGV3DError(f"Attention: {name} has {tab.shape[0]} rows, a {window[0]} x {window[1]} window needs "
                                      f"{2 * win - 1}: {_lib.REL_POS_NOT_BUILT}")
    act = torch.bfloat16 if x.dtype == torch.bfloat16 else None
    qkv = _packed(attn._pqkv, x.contiguous(), attn.qkv.weight, attn.qkv.bias, out_dtype=act)
    a = vit_grad.attention(qkv, attn.num_heads, window, attn.qkv.bias, *rel)
    return _packed(attn._pproj, a, attn.proj.weight, attn.proj.bias, residual)


def block_forward(blk, x):
    """``Block.forward``: x + attention(norm1(x)), then x + mlp(norm2(x))."""
    _require(x, "vit_train.block_forward")
    _covers(blk.attn.qkv.in_features, blk.attn.num_heads, "vit_train.block_forward")
    x = x.contiguous()
    window = (blk.window_size, blk.window_size) if blk.window_size > 0 else None
    mlp = blk.mlp
    # the bf16 mode: everything between the two residual adds is a bf16 tensor, as in Block.forward with hip_ops.VIT_BF16
    act = torch.bfloat16 if hip_ops.vit_train_bf16_active(blk.attn.qkv.in_features, blk.attn.num_heads, mlp.lin1.out_features) else None
    x = attention_forward(blk.attn, vit_grad.layer_norm(x, *_norm_params(blk.norm1), out_dtype=act), window, residual=x)
    h = vit_grad.gelu(_packed(mlp._p1, vit_grad.layer_norm(x, *_norm_params(blk.norm2), out_dtype=act), mlp.lin1.weight, mlp.lin1.bias,
                              out_dtype=act))
    return _packed(mlp._p2, h, mlp.lin2.weight, mlp.lin2.bias, x)


def _neck_output(enc, x, what):
    _require(x, what, image=True)
    if enc.pixel_mean.device != x.device or enc.patch_embed.proj.weight.device != x.device:
        raise _lib.SGV3DError(f"{what}: parameters on {enc.patch_embed.proj.weight.device}, input on {x.device}")
    for blk in enc.blocks:
        _covers(blk.attn.qkv.in_features, blk.attn.num_heads, what)
    c = enc.patch_embed.proj
    if c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1] or c.padding[0] != c.padding[1]:
        raise NotImplementedError("PatchEmbed: square kernels, strides and paddings only")
    with torch.no_grad():
        x = enc.batch_preprocess(x)
    pos = None if enc.pos_embed is None else enc.pos_embed.expand(int(x.shape[0]), -1, -1, -1).contiguous()
    x = _packed(enc.patch_embed._p, x, c.weight, c.bias, pos, stride=c.stride[0], pad=c.padding[0], cin_pad=int(x.shape[-1]))
    for blk in enc.blocks:
        x = block_forward(blk, x)
    x = _packed(enc._neck1, x, enc.neck[0].weight)
    x = vit_grad.layer_norm(x, enc.neck[1].weight, enc.neck[1].bias, enc.neck[1].eps)
    x = _packed(enc._neck2, x, enc.neck[2].weight, pad=1)
    return vit_grad.layer_norm(x, enc.neck[3].weight, enc.neck[3].bias, enc.neck[3].eps)


def encoder_forward(enc, x):
    """``ImageEncoderViT.forward``: [B, 3, H, W] with long side ``img_size`` -> the [B, out_chans, h, w] view of the cropped, resized
    NHWC neck output."""
    x = _neck_output(enc, x, "vit_train.encoder_forward")
    return vit_grad.resize_bilinear(x, enc.input_size, enc.out_dim).permute(0, 3, 1, 2)


def encoder_embed(enc, x):
    """``ImageEncoderViT.embed``: the NHWC neck output [B, img_size / p, img_size / p, out_chans]."""
    return _neck_output(enc, x, "vit_train.encoder_embed")
