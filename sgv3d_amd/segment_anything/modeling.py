"""SAM's module tree beside the image encoder: ``Sam``, ``PromptEncoder``, ``TwoWayTransformer``, ``MaskDecoder`` with the class
names, constructor signatures and parameter / buffer names of the ``segment_anything`` package, so that
``sam.load_state_dict(torch.load("sam_vit_h_4b8939.pth"))`` loads strictly by name.  Inference only, on the device, box prompts.

  tokens         sgv3d_sam_prompt_tokens: [iou_token, mask_tokens, pe(corner) + point_embeddings[2 / 3]] of every box, one launch
  src            sgv3d_sam_gather_add: image_embedding[frame of the box] + no_mask_embed (the embedding is read by index)
  projections    PackedConv (bias as shift); ``queries + qpe`` and ``keys + kpe`` are never formed: W (x + pe) = W x + W pe, and
                 W pe enters through the projection's residual input -- W kpe is a constant of the weights, kept per parameter
                 version and batch; W qpe is one small bias-free projection of the initial tokens per use
  attention      sgv3d_sam_attention (one side has 7 rows)
  MLPs           PackedConv with ReLU in the epilogue, residual in lin2's epilogue; sgv3d_layernorm
  upscaling      the k = stride transposed convolutions of PackedConv, LayerNorm2d on the NHWC map, sgv3d_gelu
  hypernetwork   sgv3d_sam_hyper_product: its weights are activations per box, which no packed-weight kernel takes

Tokens are [B, 1, N, C] NHWC maps, the image map is [B, h, w, C].
"""
from typing import List, Tuple, Type

import torch
from torch import nn

from .. import _lib, hip_ops
from ..layers.backbones.common import LayerNorm2d, PackedParam, gelu_, layernorm
from ..layers.backbones.sam_encoder import ImageEncoderViT
from . import ops


def _params_on(module, device, what):
    p = next(module.parameters())
    if p.device != device:
        raise _lib.SGV3DError(f"{what}: parameters on {p.device}, input on {device}")


def _ln(x, norm):
    return layernorm(x, norm.weight, norm.bias, norm.eps)


class _Const:
    """A tensor derived from parameters, made again when one of them (address, version, device) or ``extra`` changes."""

    def __init__(self):
        self._key = self._val = None

    def get(self, tensors, extra, build):
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in tensors) + tuple(extra)
        if key != self._key:
            self._val, self._key = build(), key
        return self._val


class MLPBlock(nn.Module):
    """lin2(act(lin1(x))) of the two-way transformer: ReLU, which the projection's epilogue applies."""

    def __init__(self, embedding_dim: int, mlp_dim: int, act: Type[nn.Module] = nn.ReLU) -> None:
        super().__init__()
        self.lin1 = nn.Linear(embedding_dim, mlp_dim)
        self.lin2 = nn.Linear(mlp_dim, embedding_dim)
        self.act = act()
        if not isinstance(self.act, nn.ReLU):
            raise NotImplementedError("MLPBlock of the mask decoder: only nn.ReLU is built")
        self._p1, self._p2 = PackedParam(), PackedParam()

    def forward(self, x, residual=None):
        ops.require_f32(x, "MLPBlock")
        with torch.no_grad():
            h = self._p1.get(self.lin1.weight, self.lin1.bias, relu=True)(x)
            return self._p2.get(self.lin2.weight, self.lin2.bias)(h, residual=residual)


class MLP(nn.Module):
    """Linear layers with ReLU between (the hypernetwork MLPs and the IoU head)."""

    def __init__(self, input_dim: int, hidden_dim: int, output_dim: int, num_layers: int, sigmoid_output: bool = False) -> None:
        super().__init__()
        if sigmoid_output:
            raise NotImplementedError("MLP: sigmoid_output is not built")
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))
        self.sigmoid_output = sigmoid_output
        self._p = [PackedParam() for _ in range(num_layers)]

    def forward(self, x, x_coff=0, out=None, y_coff=0):
        """x [B, 1, 1, ld] read at channels [x_coff, x_coff + input_dim); the last layer writes ``out`` at ``y_coff`` when given."""
        ops.require_f32(x, "MLP")
        with torch.no_grad():
            for i, layer in enumerate(self.layers):
                last = i == self.num_layers - 1
                pc = self._p[i].get(layer.weight, layer.bias, relu=not last)
                x = pc(x, out if last else None, x_coff=x_coff if i == 0 else 0, y_coff=y_coff if last else 0)
            return x


class Attention(nn.Module):
    """softmax(q k^T / sqrt(head_dim)) v per head behind q / k / v projections to ``embedding_dim / downsample_rate``."""

    def __init__(self, embedding_dim: int, num_heads: int, downsample_rate: int = 1) -> None:
        super().__init__()
        self.embedding_dim = embedding_dim
        self.internal_dim = embedding_dim // downsample_rate
        self.num_heads = num_heads
        assert self.internal_dim % num_heads == 0, "num_heads must divide embedding_dim."
        self.q_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.k_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.v_proj = nn.Linear(self.internal_dim * downsample_rate, self.internal_dim)
        self.out_proj = nn.Linear(self.internal_dim, embedding_dim)
        self._pq, self._pk, self._pv, self._po = PackedParam(), PackedParam(), PackedParam(), PackedParam()
        self._pq_pe, self._pk_pe = PackedParam(), PackedParam()
        self._const = _Const()

    def q_of_pe(self, pe):
        """W_q pe (no bias): what ``q_proj(x + pe)`` adds to ``q_proj(x)``."""
        return self._pq_pe.get(self.q_proj.weight)(pe)

    def k_of_pe(self, pe):
        return self._pk_pe.get(self.k_proj.weight)(pe)

    def const_of_pe(self, which, pe, batch):
        """``q_of_pe`` / ``k_of_pe`` of a constant map ``pe`` [1, h, w, C], repeated over the batch: made once per parameter
        version, map and batch (the residual input of a projection has the output's shape)."""
        proj = self.q_proj if which == "q" else self.k_proj
        fn = self.q_of_pe if which == "q" else self.k_of_pe
        return self._const.get((proj.weight, pe), (which, batch), lambda: fn(pe).expand(batch, -1, -1, -1).contiguous())

    def forward(self, q, k, v, q_res=None, k_res=None, residual=None):
        """q [B, hq, wq, C], k, v [B, hk, wk, C] NHWC.  ``q_res`` / ``k_res``: W pe of the positional encoding that the caller
        would have added to q / k; ``residual`` is added in out_proj's epilogue.  Returns [B, hq, wq, C]."""
        ops.require_f32(q, "Attention")
        with torch.no_grad():
            b, hq, wq, _ = (int(s) for s in q.shape)
            nk = int(k.shape[1]) * int(k.shape[2])
            qq = self._pq.get(self.q_proj.weight, self.q_proj.bias)(q, residual=q_res)
            kk = self._pk.get(self.k_proj.weight, self.k_proj.bias)(k, residual=k_res)
            vv = self._pv.get(self.v_proj.weight, self.v_proj.bias)(v)
            c = self.internal_dim
            a = ops.sam_attention(qq.view(b, hq * wq, c), kk.view(b, nk, c), vv.view(b, nk, c), self.num_heads)
            return self._po.get(self.out_proj.weight, self.out_proj.bias)(a.view(b, hq, wq, c), residual=residual)


class TwoWayAttentionBlock(nn.Module):
    def __init__(self, embedding_dim: int, num_heads: int, mlp_dim: int = 2048, activation: Type[nn.Module] = nn.ReLU,
                 attention_downsample_rate: int = 2, skip_first_layer_pe: bool = False) -> None:
        super().__init__()
        self.self_attn = Attention(embedding_dim, num_heads)
        self.norm1 = nn.LayerNorm(embedding_dim)
        self.cross_attn_token_to_image = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate)
        self.norm2 = nn.LayerNorm(embedding_dim)
        self.mlp = MLPBlock(embedding_dim, mlp_dim, activation)
        self.norm3 = nn.LayerNorm(embedding_dim)
        self.norm4 = nn.LayerNorm(embedding_dim)
        self.cross_attn_image_to_token = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate)
        self.skip_first_layer_pe = skip_first_layer_pe

    def forward(self, queries, keys, query_pe, key_pe):
        """queries, query_pe [B, 1, N, C]; keys [B, h, w, C]; key_pe [1, h, w, C] (a constant of the prompt encoder)."""
        b = int(keys.shape[0])
        sa, t2i, i2t = self.self_attn, self.cross_attn_token_to_image, self.cross_attn_image_to_token
        if self.skip_first_layer_pe:
            queries = sa(queries, queries, queries)
        else:
            queries = sa(queries, queries, queries, q_res=sa.q_of_pe(query_pe), k_res=sa.k_of_pe(query_pe), residual=queries)
        queries = _ln(queries, self.norm1)
        queries = t2i(queries, keys, keys, q_res=t2i.q_of_pe(query_pe), k_res=t2i.const_of_pe("k", key_pe, b), residual=queries)
        queries = _ln(queries, self.norm2)
        queries = _ln(self.mlp(queries, residual=queries), self.norm3)
        keys = i2t(keys, queries, queries, q_res=i2t.const_of_pe("q", key_pe, b), k_res=i2t.k_of_pe(query_pe), residual=keys)
        keys = _ln(keys, self.norm4)
        return queries, keys


class TwoWayTransformer(nn.Module):
    def __init__(self, depth: int, embedding_dim: int, num_heads: int, mlp_dim: int, activation: Type[nn.Module] = nn.ReLU,
                 attention_downsample_rate: int = 2) -> None:
        super().__init__()
        self.depth = depth
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.mlp_dim = mlp_dim
        self.attention_downsample_rate = attention_downsample_rate
        self.layers = nn.ModuleList(
            TwoWayAttentionBlock(embedding_dim=embedding_dim, num_heads=num_heads, mlp_dim=mlp_dim, activation=activation,
                                 attention_downsample_rate=attention_downsample_rate, skip_first_layer_pe=(i == 0))
            for i in range(depth))
        self.final_attn_token_to_image = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate)
        self.norm_final_attn = nn.LayerNorm(embedding_dim)

    def covered(self):
        return hip_ops.sam_decoder_covers(self.embedding_dim, self.num_heads, self.attention_downsample_rate)

    def forward(self, image_embedding, image_pe, point_embedding):
        """image_embedding [B, h, w, C] (src, per box), image_pe [1, h, w, C], point_embedding [B, 1, N, C] (the tokens).
        Returns (queries [B, 1, N, C], keys [B, h, w, C])."""
        ops.require_f32(image_embedding, "TwoWayTransformer")
        ops.require_f32(point_embedding, "TwoWayTransformer")
        if not self.covered():
            raise _lib.SGV3DError(f"TwoWayTransformer: embedding_dim {self.embedding_dim}, {self.num_heads} heads, downsample rate "
                                  f"{self.attention_downsample_rate} is not covered (hip_ops.sam_decoder_covers)")
        with torch.no_grad():
            queries, keys = point_embedding, image_embedding
            for layer in self.layers:
                queries, keys = layer(queries, keys, point_embedding, image_pe)
            fa = self.final_attn_token_to_image
            queries = fa(queries, keys, keys, q_res=fa.q_of_pe(point_embedding), k_res=fa.const_of_pe("k", image_pe, int(keys.shape[0])),
                         residual=queries)
            return _ln(queries, self.norm_final_attn), keys


class PositionEmbeddingRandom(nn.Module):
    def __init__(self, num_pos_feats: int = 64, scale: float = None) -> None:
        super().__init__()
        if scale is None or scale <= 0.0:
            scale = 1.0
        self.register_buffer("positional_encoding_gaussian_matrix", scale * torch.randn((2, num_pos_feats)))
        self._grid = _Const()

    def forward(self, size: Tuple[int, int]) -> torch.Tensor:
        """The grid's encoding as the NHWC map [1, h, w, 2 * num_pos_feats], kept per buffer version and size."""
        g = self.positional_encoding_gaussian_matrix
        if not g.is_cuda:
            raise _lib.SGV3DError("PositionEmbeddingRandom: the module must be on the GPU (there is no CPU fallback)")
        return self._grid.get((g,), tuple(size), lambda: ops.dense_pe(g.contiguous(), size[0], size[1]))


class PromptEncoder(nn.Module):
    def __init__(self, embed_dim: int, image_embedding_size: Tuple[int, int], input_image_size: Tuple[int, int], mask_in_chans: int,
                 activation: Type[nn.Module] = nn.GELU) -> None:
        super().__init__()
        self.embed_dim = embed_dim
        self.input_image_size = input_image_size
        self.image_embedding_size = image_embedding_size
        self.pe_layer = PositionEmbeddingRandom(embed_dim // 2)
        self.num_point_embeddings = 4
        self.point_embeddings = nn.ModuleList(nn.Embedding(1, embed_dim) for _ in range(self.num_point_embeddings))
        self.not_a_point_embed = nn.Embedding(1, embed_dim)
        self.mask_input_size = (4 * image_embedding_size[0], 4 * image_embedding_size[1])
        # held for loading only: mask prompts are not built
        self.mask_downscaling = nn.Sequential(
            nn.Conv2d(1, mask_in_chans // 4, kernel_size=2, stride=2),
            LayerNorm2d(mask_in_chans // 4),
            activation(),
            nn.Conv2d(mask_in_chans // 4, mask_in_chans, kernel_size=2, stride=2),
            LayerNorm2d(mask_in_chans),
            activation(),
            nn.Conv2d(mask_in_chans, embed_dim, kernel_size=1),
        )
        self.no_mask_embed = nn.Embedding(1, embed_dim)

    def get_dense_pe_nhwc(self) -> torch.Tensor:
        return self.pe_layer(self.image_embedding_size)

    def get_dense_pe(self) -> torch.Tensor:
        """[1, embed_dim, h, w], a permuted view of the NHWC map."""
        return self.get_dense_pe_nhwc().permute(0, 3, 1, 2)

    def box_tokens(self, boxes, iou_token, mask_tokens):
        """boxes [B, 4] in the input frame -> the decoder's tokens [B, 1, 7, embed_dim]: [iou_token, mask_tokens, corner 0, corner 1]."""
        ops.require_f32(boxes, "PromptEncoder")
        _params_on(self, boxes.device, "PromptEncoder")
        if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] == 0:
            raise _lib.SGV3DError(f"PromptEncoder: boxes [B, 4] with B > 0 expected, got {tuple(boxes.shape)}")
        with torch.no_grad():
            t = ops.prompt_tokens(boxes, self.input_image_size, self.pe_layer.positional_encoding_gaussian_matrix.contiguous(),
                                  self.point_embeddings[2].weight, self.point_embeddings[3].weight, iou_token, mask_tokens)
        return t.view(t.shape[0], 1, 7, self.embed_dim)

    def forward(self, points, boxes, masks):
        """(sparse [B, 2, embed_dim], dense [B, embed_dim, h, w]) for box prompts; ``dense`` is no_mask_embed as a broadcast view."""
        if points is not None:
            raise NotImplementedError("PromptEncoder: points (point prompts) are not built; the reference only passes boxes")
        if masks is not None:
            raise NotImplementedError("PromptEncoder: masks (mask prompts) are not built; the reference only passes boxes")
        if boxes is None:
            raise NotImplementedError("PromptEncoder: a boxes prompt is required")
        zeros = torch.zeros(1, self.embed_dim, device=boxes.device)
        t = self.box_tokens(boxes.reshape(-1, 4), zeros, zeros.expand(4, -1).contiguous())
        h, w = self.image_embedding_size
        dense = self.no_mask_embed.weight.detach().reshape(1, -1, 1, 1).expand(t.shape[0], -1, h, w)
        return t[:, 0, 5:], dense


class MaskDecoder(nn.Module):
    def __init__(self, transformer_dim: int, transformer: nn.Module, num_multimask_outputs: int = 3,
                 activation: Type[nn.Module] = nn.GELU, iou_head_depth: int = 3, iou_head_hidden_dim: int = 256) -> None:
        super().__init__()
        if num_multimask_outputs != 3:
            raise NotImplementedError("MaskDecoder: num_multimask_outputs must be 3 (four mask tokens)")
        if activation is not nn.GELU:
            raise NotImplementedError("MaskDecoder: only the exact nn.GELU has a kernel")
        self.transformer_dim = transformer_dim
        self.transformer = transformer
        self.num_multimask_outputs = num_multimask_outputs
        self.iou_token = nn.Embedding(1, transformer_dim)
        self.num_mask_tokens = num_multimask_outputs + 1
        self.mask_tokens = nn.Embedding(self.num_mask_tokens, transformer_dim)
        self.output_upscaling = nn.Sequential(
            nn.ConvTranspose2d(transformer_dim, transformer_dim // 4, kernel_size=2, stride=2),
            LayerNorm2d(transformer_dim // 4),
            activation(),
            nn.ConvTranspose2d(transformer_dim // 4, transformer_dim // 8, kernel_size=2, stride=2),
            activation(),
        )
        self.output_hypernetworks_mlps = nn.ModuleList(
            MLP(transformer_dim, transformer_dim, transformer_dim // 8, 3) for _ in range(self.num_mask_tokens))
        self.iou_prediction_head = MLP(transformer_dim, iou_head_hidden_dim, self.num_mask_tokens, iou_head_depth)
        self._up0, self._up3 = PackedParam(), PackedParam()

    def forward(self, image_embeddings, frame_of_box, image_pe, tokens, dense_prompt_embedding, multimask_output):
        """image_embeddings [F, h, w, C] NHWC, frame_of_box i32 [B] on the device (every entry in [0, F), checked by the caller),
        image_pe [1, h, w, C], tokens [B, 1, 7, C] (``PromptEncoder.box_tokens``), dense_prompt_embedding [C] (no_mask_embed).
        Returns (low-res masks [B, n, 4h, 4w], iou predictions [B, n]), n = 3 with ``multimask_output`` else 1."""
        ops.require_f32(image_embeddings, "MaskDecoder")
        ops.require_f32(tokens, "MaskDecoder")
        _params_on(self, image_embeddings.device, "MaskDecoder")
        d = self.transformer_dim
        if int(image_embeddings.shape[-1]) != d or int(tokens.shape[-1]) != d:
            raise _lib.SGV3DError(f"MaskDecoder: transformer_dim {d}, embedding {tuple(image_embeddings.shape)}, tokens {tuple(tokens.shape)}")
        with torch.no_grad():
            b = int(tokens.shape[0])
            src = ops.gather_add(image_embeddings, frame_of_box, dense_prompt_embedding)
            hs, keys = self.transformer(src, image_pe, tokens)
            up = self.output_upscaling
            x = self._up0.get(up[0].weight, up[0].bias, stride=2, transposed=True)(keys)
            x = gelu_(up[1].forward_nhwc(x))
            x = gelu_(self._up3.get(up[3].weight, up[3].bias, stride=2, transposed=True)(x))
            which = (1, 2, 3) if multimask_output else (0,)
            c8 = d // 8
            flat = hs.view(b, 1, 1, 7 * d)
            hyper = torch.empty(b, 1, 1, len(which) * c8, dtype=torch.float32, device=hs.device)
            for j, i in enumerate(which):
                self.output_hypernetworks_mlps[i](flat, x_coff=(1 + i) * d, out=hyper, y_coff=j * c8)
            masks = ops.hyper_product(hyper.view(b, len(which), c8), x)
            iou = self.iou_prediction_head(flat, x_coff=0).view(b, self.num_mask_tokens)
            return masks, (iou[:, 1:] if multimask_output else iou[:, 0:1])


class Sam(nn.Module):
    mask_threshold: float = 0.0
    image_format: str = "RGB"

    def __init__(self, image_encoder: ImageEncoderViT, prompt_encoder: PromptEncoder, mask_decoder: MaskDecoder,
                 pixel_mean: List[float] = [123.675, 116.28, 103.53], pixel_std: List[float] = [58.395, 57.12, 57.375]) -> None:
        super().__init__()
        self.image_encoder = image_encoder
        self.prompt_encoder = prompt_encoder
        self.mask_decoder = mask_decoder
        self.register_buffer("pixel_mean", torch.Tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.Tensor(pixel_std).view(-1, 1, 1), False)

    @property
    def device(self):
        return self.pixel_mean.device

    def forward(self, batched_input, multimask_output):
        raise NotImplementedError("Sam.forward (batched dict input) is not built: use SamPredictor")

    def postprocess_masks(self, masks, input_size, original_size):
        """[B, n, low, low] -> float [B, n, H, W]: bilinear to the square, crop to ``input_size``, bilinear to ``original_size`` --
        composed, 16 taps per pixel (sgv3d_sam_mask_compose, logit mode)."""
        ops.require_f32(masks, "Sam.postprocess_masks")
        b, n, low, _ = (int(s) for s in masks.shape)
        out = ops.mask_compose(ops.COMPOSE_LOGIT, masks.view(b * n, low, low), self.image_encoder.img_size, input_size, original_size)
        return out.view(b, n, int(original_size[0]), int(original_size[1]))
