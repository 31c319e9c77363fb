"""SAM's ViT image encoder: the reference's layers/backbones/sam_encoder.py with the same class names, constructor
signatures and parameter / buffer names, so that ``load_state_dict(get_image_encoder(sam_checkpoint))`` loads a SAM
checkpoint by name.  Inference only, on the device:

  batch_preprocess   sgv3d_vit_preprocess: (x - mean) / std, zero-padded to the square, NHWC with four channels
  patch embedding    PackedConv (patchify), ``pos_embed`` added through its residual input
  Block              sgv3d_layernorm, qkv PackedConv, sgv3d_vit_attention (windows, padding tokens and the decomposed
                     relative position inside ONE launch), proj PackedConv + shortcut, sgv3d_layernorm, lin1 PackedConv,
                     sgv3d_gelu, lin2 PackedConv + shortcut: eight launches
  neck               1x1 PackedConv, LayerNorm2d, 3x3 PackedConv, LayerNorm2d (sgv3d_layernorm on the NHWC map)
  batch_postprocess  sgv3d_resize_bilinear: crop, then bilinear to final_dim // downsample_factor

Tokens are [B, H, W, C] as in the reference, which is this project's NHWC.  The window partition is never materialised:
the attention kernel indexes the windows of the un-partitioned qkv map itself and takes the qkv BIAS as q, k, v of the
padding tokens (the reference zero-pads the normed map before the qkv linear).  The relative-position tables must have
the length 2 * size - 1 this constructor gives them; the reference's interpolation branch is not built.

bf16 mode (hip_ops.VIT_BF16 with hip_ops.MFMA_BF16, on the shapes hip_ops.vit_bf16_covers names): between the two residual adds
of a Block every tensor is bf16 in HBM -- sgv3d_layernorm_bf16out, qkv bf16 -> bf16, sgv3d_vit_attention_bf16, proj bf16 -> f32 +
shortcut, sgv3d_layernorm_bf16out, lin1 bf16 -> bf16, sgv3d_gelu_bf16, lin2 bf16 -> f32 + shortcut: still eight launches.  The
residual stream, the patch embedding, the neck, preprocess and resize keep f32 tensors.
"""
import ctypes
from functools import partial
from typing import List, Optional, Tuple, Type

import torch
from torch import nn

from ... import _lib, hip_ops
from .common import LayerNorm2d, MLPBlock, PackedParam, layernorm, require_device


def vit_attention(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None, out=None):
    """qkv [B, H, W, 3 * C] (last dimension ordered (3, heads, head_dim)) -> softmax(q k^T + rel-pos) v as [B, H, W, C],
    per ``window`` = (win_h, win_w) with the map padded up to whole windows by ``pad_qkv`` tokens (None: zeros)."""
    assert qkv.is_contiguous() and qkv.dtype == torch.float32 and qkv.dim() == 4 and qkv.shape[-1] % (3 * num_heads) == 0
    b, h, w, c3 = (int(s) for s in qkv.shape)
    c = c3 // 3
    d = _lib.vit_attn_desc(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w)
    if pad_qkv is not None:
        assert pad_qkv.is_contiguous()
    if out is None:
        out = torch.empty(b, h, w, c, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    with torch.cuda.device(qkv.device):
        rc = lib.sgv3d_vit_attention(ctypes.byref(d), qkv.data_ptr(), _lib.ptr(pad_qkv), _lib.ptr(rel_pos_h), _lib.ptr(rel_pos_w),
                                     out.data_ptr(), _lib.stream_handle(qkv.device))
    _lib.check(rc, "sgv3d_vit_attention")
    return out


def vit_attention_bf16(qkv, num_heads, window, pad_qkv=None, rel_pos_h=None, rel_pos_w=None, out=None):
    """``vit_attention`` on bf16 tensors (sgv3d_vit_attention_bf16): qkv bf16 [B, H, W, 3 * C] -> bf16 [B, H, W, C].  ``pad_qkv`` and
    the tables stay the f32 parameters; the kernel rounds them to bf16 on the way in."""
    assert qkv.is_contiguous() and qkv.dtype == torch.bfloat16 and qkv.dim() == 4 and qkv.shape[-1] % (3 * num_heads) == 0
    b, h, w, c3 = (int(s) for s in qkv.shape)
    c = c3 // 3
    d = _lib.vit_attn_desc(qkv, num_heads, window, pad_qkv, rel_pos_h, rel_pos_w)
    for t in (pad_qkv, rel_pos_h, rel_pos_w):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    if out is None:
        out = torch.empty(b, h, w, c, dtype=torch.bfloat16, device=qkv.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (b, h, w, c)
    lib = _lib.load()
    with torch.cuda.device(qkv.device):
        rc = lib.sgv3d_vit_attention_bf16(ctypes.byref(d), qkv.data_ptr(), _lib.ptr(pad_qkv), _lib.ptr(rel_pos_h), _lib.ptr(rel_pos_w),
                                          out.data_ptr(), _lib.stream_handle(qkv.device))
    _lib.check(rc, "sgv3d_vit_attention_bf16")
    return out


def vit_preprocess(img, mean, std, size):
    """[B, 3, H, W] -> normalised, zero-padded [B, size, size, 4] NHWC (channel 3 zero)."""
    b, _, h, w = (int(s) for s in img.shape)
    y = torch.empty(b, size, size, 4, dtype=torch.float32, device=img.device)
    lib = _lib.load()
    with torch.cuda.device(img.device):
        rc = lib.sgv3d_vit_preprocess(b, h, w, img.data_ptr(), mean.data_ptr(), std.data_ptr(), int(size), y.data_ptr(),
                                      _lib.stream_handle(img.device))
    _lib.check(rc, "sgv3d_vit_preprocess")
    return y


def resize_bilinear(x, crop, size):
    """NHWC x[:, :crop[0], :crop[1]] -> F.interpolate(mode='bilinear', align_corners=False) to ``size``, NHWC."""
    assert x.is_contiguous() and x.dtype == torch.float32
    b, h, w, c = (int(s) for s in x.shape)
    y = torch.empty(b, int(size[0]), int(size[1]), c, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        rc = lib.sgv3d_resize_bilinear(b, h, w, c, int(crop[0]), int(crop[1]), int(size[0]), int(size[1]), x.data_ptr(),
                                       y.data_ptr(), _lib.stream_handle(x.device))
    _lib.check(rc, "sgv3d_resize_bilinear")
    return y


def _norm_params(norm):
    if not all(hasattr(norm, a) for a in ("weight", "bias", "eps")) or norm.weight is None or norm.bias is None:
        raise NotImplementedError(f"norm_layer must be an affine LayerNorm, got {type(norm).__name__}")
    return norm.weight, norm.bias, norm.eps


class ImageEncoderViT(nn.Module):
    def __init__(
        self,
        img_size: int = 1024,
        patch_size: int = 16,
        in_chans: int = 3,
        embed_dim: int = 768,
        depth: int = 12,
        num_heads: int = 12,
        mlp_ratio: float = 4.0,
        out_chans: int = 256,
        qkv_bias: bool = True,
        norm_layer: Type[nn.Module] = nn.LayerNorm,
        act_layer: Type[nn.Module] = nn.GELU,
        use_abs_pos: bool = True,
        use_rel_pos: bool = False,
        rel_pos_zero_init: bool = True,
        window_size: int = 0,
        global_attn_indexes: Tuple[int, ...] = (),
        final_dim: tuple = (864, 1536),
        downsample_factor: int = 16,
        pixel_mean: List[float] = [123.675, 116.28, 103.53],
        pixel_std: List[float] = [58.395, 57.12, 57.375],
    ) -> None:
        super().__init__()
        if in_chans != 3:
            raise NotImplementedError("ImageEncoderViT: batch_preprocess asserts three input channels")
        self.img_size = img_size
        self.register_buffer("pixel_mean", torch.Tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.Tensor(pixel_std).view(-1, 1, 1), False)
        # the crop is the reference's: a 576 x 1024 image inside the square, whatever img_size is
        self.input_size = (576 // downsample_factor, 1024 // downsample_factor)
        self.inter_dim = (int(img_size // downsample_factor), int(img_size // downsample_factor))
        self.out_dim = (int(final_dim[0] // downsample_factor), int(final_dim[1] // downsample_factor))

        self.patch_embed = PatchEmbed(kernel_size=(patch_size, patch_size), stride=(patch_size, patch_size), in_chans=in_chans,
                                      embed_dim=embed_dim)
        self.pos_embed: Optional[nn.Parameter] = None
        if use_abs_pos:
            self.pos_embed = nn.Parameter(torch.zeros(1, img_size // patch_size, img_size // patch_size, embed_dim))

        self.blocks = nn.ModuleList()
        for i in range(depth):
            self.blocks.append(Block(
                dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer,
                act_layer=act_layer, use_rel_pos=use_rel_pos, rel_pos_zero_init=rel_pos_zero_init,
                window_size=window_size if i not in global_attn_indexes else 0,
                input_size=(img_size // patch_size, img_size // patch_size)))

        self.neck = nn.Sequential(
            nn.Conv2d(embed_dim, out_chans, kernel_size=1, bias=False),
            LayerNorm2d(out_chans),
            nn.Conv2d(out_chans, out_chans, kernel_size=3, padding=1, bias=False),
            LayerNorm2d(out_chans),
        )
        self._neck1, self._neck2 = PackedParam(), PackedParam()
        self._pos = (None, None)      # (key, pos_embed repeated over the batch): the patch embedding's residual input

    # ---- the three stages of the reference's forward, on NHWC device buffers ----
    def batch_preprocess(self, x: torch.Tensor) -> torch.Tensor:
        """Normalise and zero-pad to the square: [B, 3, H, W] -> NHWC [B, img_size, img_size, 4] (channel 3 zero)."""
        assert (
            len(x.shape) == 4
            and x.shape[1] == 3
            and max(*x.shape[2:]) == self.img_size
        ), f"set_torch_image input must be BCHW with long side {self.img_size}."
        return vit_preprocess(x.contiguous(), self.pixel_mean, self.pixel_std, self.img_size)

    def batch_postprocess(self, x: torch.Tensor) -> torch.Tensor:
        """NHWC neck output -> crop to ``input_size``, bilinear to ``out_dim``; returns the [B, C, oh, ow] view."""
        return resize_bilinear(x, self.input_size, self.out_dim).permute(0, 3, 1, 2)

    def _pos_residual(self, batch):
        p = self.pos_embed
        key = (p.data_ptr(), p._version, str(p.device), batch)
        if self._pos[0] != key:
            self._pos = (key, p.detach().expand(batch, -1, -1, -1).contiguous())
        return self._pos[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        require_device(x, "ImageEncoderViT")
        if self.pixel_mean.device != x.device or self.patch_embed.proj.weight.device != x.device:
            raise _lib.SGV3DError(f"ImageEncoderViT: parameters on {self.patch_embed.proj.weight.device}, input on {x.device}")
        with torch.no_grad():
            x = self.batch_preprocess(x)
            x = self.patch_embed(x, residual=None if self.pos_embed is None else self._pos_residual(int(x.shape[0])))
            for blk in self.blocks:
                x = blk(x)
            x = self._neck1.get(self.neck[0].weight)(x)
            x = self.neck[1].forward_nhwc(x)
            x = self._neck2.get(self.neck[2].weight, pad=1)(x)
            x = self.neck[3].forward_nhwc(x)
            return self.batch_postprocess(x)

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        """SAM's own forward, without the reference's crop and resize: [B, 3, H, W] with long side ``img_size`` -> the NHWC neck
        output [B, img_size / 16, img_size / 16, out_chans] that the mask decoder of sgv3d_amd.segment_anything reads."""
        require_device(x, "ImageEncoderViT")
        if self.pixel_mean.device != x.device or self.patch_embed.proj.weight.device != x.device:
            raise _lib.SGV3DError(f"ImageEncoderViT: parameters on {self.patch_embed.proj.weight.device}, input on {x.device}")
        with torch.no_grad():
            x = self.batch_preprocess(x)
            x = self.patch_embed(x, residual=None if self.pos_embed is None else self._pos_residual(int(x.shape[0])))
            for blk in self.blocks:
                x = blk(x)
            x = self._neck1.get(self.neck[0].weight)(x)
            x = self.neck[1].forward_nhwc(x)
            x = self._neck2.get(self.neck[2].weight, pad=1)(x)
            return self.neck[3].forward_nhwc(x)


class Block(nn.Module):
    """Transformer block with window attention (``window_size`` > 0) or global attention (0)."""

    def __init__(
        self,
        dim: int,
        num_heads: int,
        mlp_ratio: float = 4.0,
        qkv_bias: bool = True,
        norm_layer: Type[nn.Module] = nn.LayerNorm,
        act_layer: Type[nn.Module] = nn.GELU,
        use_rel_pos: bool = False,
        rel_pos_zero_init: bool = True,
        window_size: int = 0,
        input_size: Optional[Tuple[int, int]] = None,
    ) -> None:
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, use_rel_pos=use_rel_pos,
                              rel_pos_zero_init=rel_pos_zero_init,
                              input_size=input_size if window_size == 0 else (window_size, window_size))
        self.norm2 = norm_layer(dim)
        self.mlp = MLPBlock(embedding_dim=dim, mlp_dim=int(dim * mlp_ratio), act=act_layer)
        self.window_size = window_size

    def bf16_mode(self) -> bool:
        """hip_ops.VIT_BF16 in bf16 compute mode on a covered shape: everything between the two residual adds is bf16 in HBM (the
        LayerNorms write bf16, qkv / attention / lin1 / GELU read and write bf16, proj and lin2 read bf16, write f32 and add the
        f32 residual).  The residual stream stays f32."""
        return hip_ops.vit_bf16_active(self.attn.qkv.in_features, self.attn.num_heads, self.mlp.lin1.out_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        require_device(x, "Block")
        with torch.no_grad():
            window = (self.window_size, self.window_size) if self.window_size > 0 else None
            act = torch.bfloat16 if self.bf16_mode() else None
            x = self.attn(layernorm(x, *_norm_params(self.norm1), out_dtype=act), window=window, residual=x)     # shortcut + attention
            return self.mlp(layernorm(x, *_norm_params(self.norm2), out_dtype=act), residual=x)                  # x + mlp(norm2(x))


class Attention(nn.Module):
    """Multi-head attention with decomposed relative position."""

    def __init__(
        self,
        dim: int,
        num_heads: int = 8,
        qkv_bias: bool = True,
        use_rel_pos: bool = False,
        rel_pos_zero_init: bool = True,
        input_size: Optional[Tuple[int, int]] = None,
    ) -> None:
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim**-0.5

        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

        self.use_rel_pos = use_rel_pos
        if self.use_rel_pos:
            assert (
                input_size is not None
            ), "Input size must be provided if using relative positional encoding."
            self.rel_pos_h = nn.Parameter(torch.zeros(2 * input_size[0] - 1, head_dim))
            self.rel_pos_w = nn.Parameter(torch.zeros(2 * input_size[1] - 1, head_dim))
        self._pqkv, self._pproj = PackedParam(), PackedParam()

    def forward(self, x: torch.Tensor, window=None, residual=None) -> torch.Tensor:
        """x [B, H, W, C], the normed map, UN-partitioned.  ``window`` (win_h, win_w): attention inside the windows of the
        map padded up to whole windows, as window_partition / window_unpartition around this module give in the
        reference; None: global.  ``residual`` is added in proj's epilogue.  A bf16 ``x`` (the encoder's bf16 mode): qkv and the
        attention output are bf16 tensors, proj writes f32."""
        _, h, w, _ = x.shape
        window = window or (int(h), int(w))
        if self.use_rel_pos:
            for name, tab, win in (("rel_pos_h", self.rel_pos_h, window[0]), ("rel_pos_w", self.rel_pos_w, window[1])):
                if tab.shape[0] != 2 * win - 1:
                    raise _lib.SGV3DError(f"Attention: {name} has {tab.shape[0]} rows, a {window[0]} x {window[1]} window needs "
                                          f"{2 * win - 1}: {_lib.REL_POS_NOT_BUILT}")
        require_device(x, "Attention", bf16_ok=True)
        with torch.no_grad():
            qkv = self._pqkv.get(self.qkv.weight, self.qkv.bias)(x, out_dtype=x.dtype)
            rel = (self.rel_pos_h.detach(), self.rel_pos_w.detach()) if self.use_rel_pos else (None, None)
            bias = None if self.qkv.bias is None else self.qkv.bias.detach()
            attend = vit_attention_bf16 if x.dtype == torch.bfloat16 else vit_attention
            a = attend(qkv, self.num_heads, window, bias, *rel)
            return self._pproj.get(self.proj.weight, self.proj.bias)(a, residual=residual)


class PatchEmbed(nn.Module):
    """Image to patch embedding."""

    def __init__(
        self,
        kernel_size: Tuple[int, int] = (16, 16),
        stride: Tuple[int, int] = (16, 16),
        padding: Tuple[int, int] = (0, 0),
        in_chans: int = 3,
        embed_dim: int = 768,
    ) -> None:
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=kernel_size, stride=stride, padding=padding)
        self._p = PackedParam()

    def forward(self, x: torch.Tensor, residual=None) -> torch.Tensor:
        """x NHWC [B, H, W, 4] (``batch_preprocess``'s output: the channels padded to four) -> tokens [B, H/p, W/p, C]."""
        require_device(x, "PatchEmbed")
        c = self.proj
        if c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1] or c.padding[0] != c.padding[1]:
            raise NotImplementedError("PatchEmbed: square kernels, strides and paddings only")
        with torch.no_grad():
            return self._p.get(c.weight, c.bias, stride=c.stride[0], pad=c.padding[0], cin_pad=int(x.shape[-1]))(x, residual=residual)


def get_image_encoder(state_dict):
    """The ``image_encoder.*`` entries of a SAM checkpoint with the prefix removed."""
    prefix = "image_encoder."
    return {k[len(prefix):]: v for k, v in state_dict.items() if "image_encoder" in k}


def _build_vit(encoder_embed_dim, encoder_depth, encoder_num_heads, encoder_global_attn_indexes, final_dim, downsample_factor,
               checkpoint=None):
    image_encoder = ImageEncoderViT(
        depth=encoder_depth,
        embed_dim=encoder_embed_dim,
        img_size=1024,
        mlp_ratio=4,
        norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
        num_heads=encoder_num_heads,
        patch_size=16,
        qkv_bias=True,
        use_rel_pos=True,
        global_attn_indexes=encoder_global_attn_indexes,
        window_size=14,
        out_chans=256,
        final_dim=final_dim,
        downsample_factor=downsample_factor,
    )
    if checkpoint is not None:
        with open(checkpoint, "rb") as f:
            state_dict = torch.load(f)
        image_encoder.load_state_dict(get_image_encoder(state_dict))
    return image_encoder


def build_sam_vit_b(final_dim, downsample_factor, checkpoint=None):
    return _build_vit(768, 12, 12, [2, 5, 8, 11], final_dim, downsample_factor, checkpoint)


def build_sam_vit_l(final_dim, downsample_factor, checkpoint=None):
    return _build_vit(1024, 24, 16, [5, 11, 17, 23], final_dim, downsample_factor, checkpoint)


def build_sam_vit_h(final_dim, downsample_factor, checkpoint=None):
    return _build_vit(1280, 32, 16, [7, 15, 23, 31], final_dim, downsample_factor, checkpoint)
