"""CPU: SAM's prompt encoder and mask decoder without a GPU -- the C ABI of csrc/sam_decoder.hip (header against ctypes, every
rejection by name before any HIP call), the coverage rule, the package's names and state-dict keys for ViT-H / L / B, the
restatement's positional encoding against closed-form values, ResizeLongestSide, Pillow's BILINEAR coefficients against the
fixture, the host compose twin against the restatement and against the reference's get_sam_mask, and the share of pixels the
float64 restatement leaves within the bar of zero on every seeded case."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sam_masks_cases as C          # noqa: E402
import sam_ref                       # noqa: E402

ENTRIES = ("sgv3d_sam_attention_workspace_bytes", "sgv3d_sam_attention", "sgv3d_sam_prompt_tokens", "sgv3d_sam_dense_pe",
           "sgv3d_sam_gather_add", "sgv3d_sam_hyper_product", "sgv3d_sam_mask_compose_workspace_bytes", "sgv3d_sam_mask_compose",
           "sgv3d_sam_mask_compose_host", "sgv3d_resize_u8_filter")
A = 4096          # a non-null, 16-byte aligned address: every call below is refused before it is looked at


def _ctype_of(decl):
    if "*" in decl:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[decl.rsplit(" ", 1)[0]]


def test_header_matches_ctypes():
    from sgv3d_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in sgv3d_hip.h"
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        res, argtypes = _lib._PROTOS[name]
        assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)]
        got = [ctypes.c_void_p if (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t for t in argtypes]
        assert got == [_ctype_of(a) for a in args], f"{name}: ctypes {got} against the header's {args}"
        assert name in _lib.EXPORTED_SYMBOLS
    fields = re.search(r"typedef struct sgv3d_sam_attn_desc \{(.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [n for n, _ in _lib.SamAttnDesc._fields_]
    assert re.search(r"#define SGV3D_FILTER_BILINEAR 2\b", text) and re.search(r"#define SGV3D_FILTER_LANCZOS 1\b", text)


def _rejected(lib, rc, word):
    msg = lib.sgv3d_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_attention_rejections_by_name():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.SamAttnDesc
    ok = dict(batch=1, nq=7, nk=300, heads=8, head_dim=16, q_ld=128, k_ld=128, v_ld=128, o_ld=128, scale=0.25)
    call = lambda d, q=A, k=A, v=A, o=A, ws=A, n=1 << 20: lib.sgv3d_sam_attention(None if d is None else ctypes.byref(D(**d)), q, k, v, o, ws, n, None)
    _rejected(lib, call(None), "null descriptor")
    _rejected(lib, call(dict(ok, nq=0)), "zero or negative dimension")
    _rejected(lib, call(dict(ok, head_dim=64)), "head_dim 64 is not one of 16, 32")
    _rejected(lib, call(dict(ok, nq=17)), "neither side is small")
    _rejected(lib, call(dict(ok, heads=70000, q_ld=1 << 21, k_ld=1 << 21, v_ld=1 << 21, o_ld=1 << 21)), "above 65535")
    _rejected(lib, call(dict(ok, k_ld=124)), "below heads * head_dim")
    _rejected(lib, call(dict(ok, o_ld=130)), "multiples of 4")
    _rejected(lib, call(dict(ok, scale=float("inf"))), "scale is not finite")
    _rejected(lib, call(ok, q=None), "null q, k, v or out")
    _rejected(lib, call(ok, v=A + 4), "16-byte aligned")
    need = lib.sgv3d_sam_attention_workspace_bytes(ctypes.byref(D(**ok)))
    assert need == 1 * 8 * 2 * 16 * 18 * 4
    _rejected(lib, call(ok, n=need - 1), "workspace")
    _rejected(lib, call(ok, ws=None), "workspace")
    assert lib.sgv3d_sam_attention_workspace_bytes(ctypes.byref(D(**dict(ok, nk=256)))) == 0
    assert lib.sgv3d_sam_attention_workspace_bytes(ctypes.byref(D(**dict(ok, nq=5000, nk=7)))) == 0
    assert lib.sgv3d_sam_attention_workspace_bytes(ctypes.byref(D(**dict(ok, head_dim=8)))) == 0


def test_other_entries_reject_by_name():
    from sgv3d_amd import _lib
    lib = _lib.load()
    _rejected(lib, lib.sgv3d_sam_prompt_tokens(0, 256, 96, 96, A, A, A, A, A, A, A, None), "non-positive size")
    _rejected(lib, lib.sgv3d_sam_prompt_tokens(1, 255, 96, 96, A, A, A, A, A, A, A, None), "is odd")
    _rejected(lib, lib.sgv3d_sam_prompt_tokens(1, 256, 96, 96, A, None, A, A, A, A, A, None), "null pointer")
    _rejected(lib, lib.sgv3d_sam_dense_pe(6, 0, 256, A, A, None), "non-positive size")
    _rejected(lib, lib.sgv3d_sam_dense_pe(6, 6, 256, A, None, None), "null pointer")
    _rejected(lib, lib.sgv3d_sam_gather_add(1, 1, 36, 255, A, A, A, A, None), "not a multiple of 4")
    _rejected(lib, lib.sgv3d_sam_gather_add(1, 0, 36, 256, A, A, A, A, None), "non-positive size")
    _rejected(lib, lib.sgv3d_sam_gather_add(1, 1, 36, 256, A, A, A + 4, A, None), "16-byte aligned")
    _rejected(lib, lib.sgv3d_sam_hyper_product(1, 576, 32, 5, 160, A, A, A, None), "n 5 above 4")
    _rejected(lib, lib.sgv3d_sam_hyper_product(1, 576, 30, 1, 30, A, A, A, None), "not a multiple of 4")
    _rejected(lib, lib.sgv3d_sam_hyper_product(1, 576, 32, 3, 64, A, A, A, None), "hyper_ld 64 below")
    _rejected(lib, lib.sgv3d_sam_hyper_product(1, 576, 32, 1, 32, A, None, A, None), "null pointer")
    big = 1 << 24
    comp = lambda *a, ws=A, n=big: lib.sgv3d_sam_mask_compose(*a, ws, n, None)
    good = (0, 2, 1, 24, 96, 54, 96, 54, 96, A, A, A, A)
    for i, word in ((0, "unknown mode"), (1, "negative box count"), (2, "non-positive frame count"), (3, "non-positive size"), (7, "non-positive size")):
        bad = list(good)
        bad[i] = -1 if i else 7
        _rejected(lib, comp(*bad), word)
    _rejected(lib, comp(*(good[:5] + (97,) + good[6:])), "exceeds the square")
    _rejected(lib, comp(*(good[:9] + (None,) + good[10:])), "null logits")
    _rejected(lib, comp(*(good[:10] + (None,) + good[11:])), "null labels or frame_of_box")
    _rejected(lib, comp(*(good[:12] + (None,))), "null output")
    _rejected(lib, comp(1, 0, 1, 24, 96, 54, 96, 54, 96, A, A, A, A), "at least one box")
    need = lib.sgv3d_sam_mask_compose_workspace_bytes(54, 96)
    assert need >= (54 + 96) * 4 * 12 and need % 256 == 0 and lib.sgv3d_sam_mask_compose_workspace_bytes(0, 96) == 0
    _rejected(lib, comp(*good, n=need - 1), "workspace")
    _rejected(lib, lib.sgv3d_sam_mask_compose_host(7, 1, 1, 24, 96, 54, 96, 54, 96, A, A, A, A), "unknown mode")
    _rejected(lib, lib.sgv3d_resize_u8_filter(1, 0, 96, 54, 96, A, A, 3, A, A, 3, 0, A, A, A, None), "non-positive size")
    _rejected(lib, lib.sgv3d_resize_u8_filter(1, 54, 96, 54, 96, A, A, 0, A, A, 3, 0, A, A, A, None), "non-positive ksize")
    _rejected(lib, lib.sgv3d_resize_u8_filter(1, 54, 96, 54, 96, A, A, 3, A, A, 3, 0, None, A, A, None), "null pointer")
    ks = ctypes.c_int(0)
    _rejected(lib, lib.sgv3d_resample_coeffs_filter(3, 10, 5, None, None, ctypes.byref(ks)), "unknown filter")


def test_coverage_rule_and_python_refusals():
    from sgv3d_amd import _lib, hip_ops, sam_masks
    from sgv3d_amd.segment_anything import SamPredictor, build_sam_hq, ops
    from sgv3d_amd.segment_anything.modeling import MaskDecoder, PromptEncoder, TwoWayTransformer
    assert hip_ops.sam_decoder_covers(256, 8, 2) and hip_ops.sam_decoder_covers(256, 8, 1) and hip_ops.sam_decoder_covers(128, 4, 2)
    for bad in ((256, 4, 2), (256, 8, 4), (128, 2, 2), (250, 5, 2), (0, 8, 2), (256, 8, 3)):
        assert not hip_ops.sam_decoder_covers(*bad), bad
    with pytest.raises(NotImplementedError, match="build_sam_hq"):
        build_sam_hq()
    pe = PromptEncoder(256, (6, 6), (96, 96), 16)
    with pytest.raises(NotImplementedError, match="points"):
        pe(torch.zeros(1, 1, 2), None, None)
    with pytest.raises(NotImplementedError, match="masks"):
        pe(None, torch.zeros(1, 4), torch.zeros(1, 1, 24, 24))
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        pe(None, torch.zeros(1, 4), None)
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        ops.sam_attention(torch.zeros(1, 7, 128), torch.zeros(1, 9, 128), torch.zeros(1, 9, 128), 8)
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        TwoWayTransformer(1, 256, 8, 64)(torch.zeros(1, 2, 2, 256), torch.zeros(1, 2, 2, 256), torch.zeros(1, 1, 7, 256))
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        ops.resize_bilinear_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2))
    with pytest.raises(_lib.SGV3DError, match="on the GPU"):
        sam_masks.mask_images(None, torch.zeros(1, 4, 4, 3, dtype=torch.uint8), [[]], [[]])
    with pytest.raises(NotImplementedError, match="num_multimask_outputs"):
        MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(1, 256, 8, 64), num_multimask_outputs=2)


def _expected_keys(embed_dim, depth, global_idx):
    """The state dict of a SAM checkpoint, spelled out: name -> shape."""
    hd = embed_dim // {768: 12, 1024: 16, 1280: 16}[embed_dim]
    e = {"pos_embed": (1, 64, 64, embed_dim), "patch_embed.proj.weight": (embed_dim, 3, 16, 16), "patch_embed.proj.bias": (embed_dim,),
         "neck.0.weight": (256, embed_dim, 1, 1), "neck.1.weight": (256,), "neck.1.bias": (256,), "neck.2.weight": (256, 256, 3, 3),
         "neck.3.weight": (256,), "neck.3.bias": (256,)}
    for i in range(depth):
        win = 64 if i in global_idx else 14
        p = f"blocks.{i}."
        e.update({p + "norm1.weight": (embed_dim,), p + "norm1.bias": (embed_dim,), p + "norm2.weight": (embed_dim,), p + "norm2.bias": (embed_dim,),
                  p + "attn.rel_pos_h": (2 * win - 1, hd), p + "attn.rel_pos_w": (2 * win - 1, hd),
                  p + "attn.qkv.weight": (3 * embed_dim, embed_dim), p + "attn.qkv.bias": (3 * embed_dim,),
                  p + "attn.proj.weight": (embed_dim, embed_dim), p + "attn.proj.bias": (embed_dim,),
                  p + "mlp.lin1.weight": (4 * embed_dim, embed_dim), p + "mlp.lin1.bias": (4 * embed_dim,),
                  p + "mlp.lin2.weight": (embed_dim, 4 * embed_dim), p + "mlp.lin2.bias": (embed_dim,)})
    out = {"image_encoder." + k: v for k, v in e.items()}
    d = 256
    pe = {"pe_layer.positional_encoding_gaussian_matrix": (2, 128), "not_a_point_embed.weight": (1, d), "no_mask_embed.weight": (1, d),
          "mask_downscaling.0.weight": (4, 1, 2, 2), "mask_downscaling.0.bias": (4,), "mask_downscaling.1.weight": (4,), "mask_downscaling.1.bias": (4,),
          "mask_downscaling.3.weight": (16, 4, 2, 2), "mask_downscaling.3.bias": (16,), "mask_downscaling.4.weight": (16,), "mask_downscaling.4.bias": (16,),
          "mask_downscaling.6.weight": (d, 16, 1, 1), "mask_downscaling.6.bias": (d,)}
    pe.update({f"point_embeddings.{i}.weight": (1, d) for i in range(4)})
    out.update({"prompt_encoder." + k: v for k, v in pe.items()})

    def attention(prefix, rate):
        c = d // rate
        return {prefix + "q_proj.weight": (c, d), prefix + "q_proj.bias": (c,), prefix + "k_proj.weight": (c, d), prefix + "k_proj.bias": (c,),
                prefix + "v_proj.weight": (c, d), prefix + "v_proj.bias": (c,), prefix + "out_proj.weight": (d, c), prefix + "out_proj.bias": (d,)}

    md = {"iou_token.weight": (1, d), "mask_tokens.weight": (4, d),
          "output_upscaling.0.weight": (d, 64, 2, 2), "output_upscaling.0.bias": (64,), "output_upscaling.1.weight": (64,), "output_upscaling.1.bias": (64,),
          "output_upscaling.3.weight": (64, 32, 2, 2), "output_upscaling.3.bias": (32,)}
    for i in range(2):
        p = f"transformer.layers.{i}."
        md.update(attention(p + "self_attn.", 1))
        md.update(attention(p + "cross_attn_token_to_image.", 2))
        md.update(attention(p + "cross_attn_image_to_token.", 2))
        for n in (1, 2, 3, 4):
            md.update({p + f"norm{n}.weight": (d,), p + f"norm{n}.bias": (d,)})
        md.update({p + "mlp.lin1.weight": (2048, d), p + "mlp.lin1.bias": (2048,), p + "mlp.lin2.weight": (d, 2048), p + "mlp.lin2.bias": (d,)})
    md.update(attention("transformer.final_attn_token_to_image.", 2))
    md.update({"transformer.norm_final_attn.weight": (d,), "transformer.norm_final_attn.bias": (d,)})
    for i in range(4):
        for j, (o, c) in enumerate(((d, d), (d, d), (32, d))):
            md.update({f"output_hypernetworks_mlps.{i}.layers.{j}.weight": (o, c), f"output_hypernetworks_mlps.{i}.layers.{j}.bias": (o,)})
    for j, (o, c) in enumerate(((256, d), (256, 256), (4, 256))):
        md.update({f"iou_prediction_head.layers.{j}.weight": (o, c), f"iou_prediction_head.layers.{j}.bias": (o,)})
    out.update({"mask_decoder." + k: v for k, v in md.items()})
    return out


@pytest.mark.parametrize("name,embed_dim,depth,global_idx", [("vit_b", 768, 12, (2, 5, 8, 11)), ("vit_l", 1024, 24, (5, 11, 17, 23)),
                                                             ("vit_h", 1280, 32, (7, 15, 23, 31))])
def test_state_dict_keys_and_shapes(name, embed_dim, depth, global_idx):
    import sgv3d_amd.segment_anything as SA
    assert SA.build_sam is SA.build_sam_vit_h and SA.sam_model_registry["default"] is SA.build_sam_vit_h
    with torch.device("meta"):
        sam = SA.sam_model_registry[name]()
    got = {k: tuple(v.shape) for k, v in sam.state_dict().items()}
    want = _expected_keys(embed_dim, depth, global_idx)
    assert set(got) == set(want), (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    assert got == want
    assert sam.mask_threshold == 0.0 and tuple(sam.pixel_mean.shape) == (3, 1, 1) and "pixel_mean" not in got
    assert isinstance(SA.SamPredictor, type) and SA.install() is sys.modules["segment_anything"]
    from segment_anything import SamPredictor, build_sam          # noqa: F401  (the reference's import line)


def test_restatement_exchanges_state_dicts_with_the_product():
    from functools import partial
    from sgv3d_amd.layers.backbones.sam_encoder import ImageEncoderViT
    from sgv3d_amd.segment_anything.modeling import MaskDecoder, PromptEncoder, Sam, TwoWayTransformer
    ref = sam_ref.randomize_(sam_ref.build(), 1)
    enc = ImageEncoderViT(img_size=96, patch_size=16, embed_dim=64, depth=2, num_heads=2, out_chans=256, use_rel_pos=True, window_size=4,
                          global_attn_indexes=(1,), norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    sam = Sam(enc, PromptEncoder(256, (6, 6), (96, 96), 16), MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(2, 256, 8, 2048)))
    sam.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(sam.state_dict(), strict=True)


def test_positional_encoding_closed_form():
    pe = sam_ref.PositionEmbeddingRandom(2).double()
    pe.positional_encoding_gaussian_matrix.copy_(torch.eye(2, dtype=torch.float64))          # unit columns: z = (2x - 1, 2y - 1)
    for x, y in ((0.5, 0.5), (0.75, 0.5), (0.625, 0.3125), (0.0, 1.0)):
        got = pe.pe(torch.tensor([x, y], dtype=torch.float64))
        a, b = 2 * math.pi * (2 * x - 1), 2 * math.pi * (2 * y - 1)
        assert torch.allclose(got, torch.tensor([math.sin(a), math.sin(b), math.cos(a), math.cos(b)], dtype=torch.float64), atol=1e-15)
    grid = pe((2, 4))                                    # [C, h, w]: point (i, j) is ((j + 0.5) / w, (i + 0.5) / h)
    assert grid.shape == (4, 2, 4)
    assert abs(grid[0, 1, 2].item() - math.sin(2 * math.pi * (2 * 2.5 / 4 - 1))) < 1e-15
    assert abs(grid[3, 1, 2].item() - math.cos(2 * math.pi * (2 * 1.5 / 2 - 1))) < 1e-15
    enc = sam_ref.PromptEncoder(4, (2, 2), (10, 20), 16).double()
    enc.pe_layer.positional_encoding_gaussian_matrix.copy_(torch.eye(2, dtype=torch.float64))
    sparse, dense = enc(torch.tensor([[4.5, 2.0, 14.5, 7.0]], dtype=torch.float64))      # corners (5 / 20, 2.5 / 10), (15 / 20, 7.5 / 10)
    want0 = torch.tensor([math.sin(-math.pi), math.sin(-math.pi), math.cos(-math.pi), math.cos(-math.pi)]) + enc.point_embeddings[2].weight[0]
    want1 = torch.tensor([math.sin(math.pi), math.sin(math.pi), math.cos(math.pi), math.cos(math.pi)]) + enc.point_embeddings[3].weight[0]
    assert torch.allclose(sparse[0, 0], want0, atol=1e-14) and torch.allclose(sparse[0, 1], want1, atol=1e-14) and dense.shape == (1, 4, 2, 2)


def test_resize_longest_side():
    from sgv3d_amd.segment_anything import ResizeLongestSide
    t = ResizeLongestSide(1024)
    assert t.get_preprocess_shape(1080, 1920, 1024) == (576, 1024) and sam_ref.get_preprocess_shape(1080, 1920, 1024) == (576, 1024)
    for h, w, L in ((135, 240, 96), (27, 48, 96), (40, 63, 96), (37, 61, 96), (1, 7, 96), (1079, 1919, 1024), (63, 40, 96)):
        nh, nw = t.get_preprocess_shape(h, w, L)
        assert (nh, nw) == sam_ref.get_preprocess_shape(h, w, L) and max(nh, nw) == L
        assert nh == int(h * (L / max(h, w)) + 0.5) and nw == int(w * (L / max(h, w)) + 0.5)
    boxes = torch.tensor([[0, 0, 1919, 1079], [100, 50, 300, 700], [3, 5, 7, 11]])
    got = t.apply_boxes_torch(boxes, (1080, 1920))
    assert got.dtype == torch.float32 and torch.equal(got, sam_ref.apply_boxes(boxes, (1080, 1920), 1024))
    want = boxes.double() * torch.tensor([1024 / 1920, 576 / 1080] * 2, dtype=torch.float64)
    assert (got.double() - want).abs().max().item() <= 1024 * 2.0 ** -23
    odd = ResizeLongestSide(96).apply_boxes_torch(torch.tensor([[1.5, 2.5, 60, 39]]), (40, 63))
    assert torch.allclose(odd.double(), torch.tensor([[1.5 * 96 / 63, 2.5 * 61 / 40, 60 * 96 / 63, 39 * 61 / 40]], dtype=torch.float64), atol=1e-5)


def test_bilinear_coefficients_against_pillow():
    from sgv3d_amd.segment_anything import ops
    z = C.golden()
    keys = [k for k in z.files if k.startswith("resize_src_")]
    assert len(keys) == 5
    for key in keys:
        tag = key[len("resize_src_"):]
        want = z["resize_out_" + tag]
        assert np.array_equal(ops.resize_bilinear_u8_host(z[key], want.shape[:2]), want), tag
    # the triangle: an upscale by two has the weights 3/4, 1/4 inside and sums to 1 << 22 everywhere
    bounds, coeffs = ops.resample_coeffs(ops.FILTER_BILINEAR, 27, 54)
    assert coeffs.shape == (54, 3) and (coeffs.sum(1) == 1 << 22).all()
    assert sorted(coeffs[10].tolist()) == [0, 1 << 20, 3 << 20] and bounds[10].tolist()[1] >= 2
    # the existing filters are as they were
    from sgv3d_amd import train_augment as TA
    b0, c0 = TA.resample_coeffs_filter(TA.FILTER_BICUBIC, 135, 54)
    assert c0.shape[1] == 2 * math.ceil(2 * 135 / 54) + 1 and (c0.sum(1) - (1 << 22)).__abs__().max() <= 8


def test_host_compose_twin_against_the_restatement():
    from sgv3d_amd.segment_anything import ops
    for hw in C.COMPOSE_SIZES + [(37, 61)]:
        logits, labels, frames, nf = C.compose_case(hw, 24)
        pre = sam_ref.get_preprocess_shape(hw[0], hw[1], 96)
        ref = sam_ref.postprocess_masks(torch.from_numpy(logits).double()[None], 96, pre, hw)[0].numpy()
        val = ops.mask_compose_host(ops.COMPOSE_LOGIT, logits, 96, pre, hw)
        assert np.abs(val - ref).max() <= 2.0 ** -23 * np.abs(ref).max() + 1e-12            # one float32 rounding of the float64 value
        masks = ops.mask_compose_host(ops.COMPOSE_BOOL, logits, 96, pre, hw)
        clear = np.abs(ref) > 1e-9
        assert np.array_equal(masks[clear], (ref > 0)[clear]) and clear.mean() > 0.999
        cls = ops.mask_compose_host(ops.COMPOSE_CLASS, logits, 96, pre, hw, labels, frames, nf)
        for f in range(nf):
            sel = [i for i, fr in enumerate(frames) if fr == f]
            assert np.array_equal(sam_ref.paint([masks[i] for i in sel], [labels[i] for i in sel], hw), cls[f])
        assert cls[1].max() == 0 and cls[2][-1, -1] == 3 and cls.max() == 6
        assert ops.mask_compose_host(ops.COMPOSE_CLASS, None, 96, pre, hw, [], [], 2).max() == 0      # no boxes: zeros


def test_paint_loop_against_the_reference_fixture():
    """The reference's own get_sam_mask on prepared masks pins the restatement's paint loop, and the host twin's class image is that
    loop over the twin's own per-box masks at the reference's 1080 x 1920 (576 x 1024 preprocess shape of the 1024 square)."""
    from sgv3d_amd.segment_anything import ops
    z = C.golden()
    rects, labels = z["paint_rects"], z["paint_labels"].tolist()
    masks = np.zeros((len(rects), 1080, 1920), bool)
    for i, (x0, y0, x1, y1) in enumerate(rects):
        masks[i, y0:y1 + 1, x0:x1 + 1] = True
    assert np.array_equal(sam_ref.paint(masks, labels, (1080, 1920)), z["paint_out"])
    assert int(z["empty_out_sum"]) == 0 and int(z["noboxes_out_sum"]) == 0 and set(np.unique(z["paint_out"])) == {0, 2, 3, 5, 6}
    low = -np.ones((len(rects), 256, 256), np.float32)
    for i, (x0, y0, x1, y1) in enumerate(rects):                      # the same rectangles at low resolution (1920 / 256 = 7.5 pixels a cell)
        low[i, int(y0 / 7.5):int(y1 / 7.5) + 1, int(x0 / 7.5):int(x1 / 7.5) + 1] = 1.0
    twin = ops.mask_compose_host(ops.COMPOSE_BOOL, low, 1024, (576, 1024), (1080, 1920))
    cls = ops.mask_compose_host(ops.COMPOSE_CLASS, low, 1024, (576, 1024), (1080, 1920), labels, [0] * len(labels), 1)[0]
    assert np.array_equal(sam_ref.paint(twin, labels, (1080, 1920)), cls)
    # the low-resolution rectangles are the fixture's up to their edges: an edge may sit anywhere in its 7.5-pixel cell, so at most
    # perimeter x 7.5 pixels of a box can differ
    edge = sum(2 * ((x1 - x0 + 1) + (y1 - y0 + 1)) * 7.5 for x0, y0, x1, y1 in rects.tolist())
    assert (cls != z["paint_out"]).sum() <= edge and edge < 0.05 * cls.size
    assert ops.mask_compose_host(ops.COMPOSE_CLASS, low[:1], 1024, (576, 1024), (1080, 1920), [0], [0], 1).max() == 0      # label 0 paints nothing


@pytest.mark.parametrize("case", C.DECODER_CASES, ids=lambda c: c.name)
def test_restatement_keeps_the_excused_pixels_under_the_cap(case):
    model, emb, boxes, frames = C.decoder_case(case)
    low64, _ = C.run_ref(model, emb, boxes, frames, torch.float64, case.multimask)
    low32, _ = C.run_ref(model, emb, boxes, frames, torch.float32, case.multimask)
    bar = 4 * (low32.double() - low64).abs().max().item()
    size = 16 * case.grid
    out = sam_ref.postprocess_masks(low64, size, sam_ref.get_preprocess_shape(case.original[0], case.original[1], size), case.original)
    share = (out.abs() <= bar).float().mean().item()
    assert 0 < bar < 1e-3 and share <= 0.005, (bar, share)
    assert 0.01 < (out > 0).float().mean().item() < 0.99          # the case has both classes of pixel


def test_whole_path_restatement_keeps_the_excused_pixels_under_the_cap():
    ref64 = sam_ref.randomize_(sam_ref.build(), C.WHOLE_SEED).double()
    frame, boxes = C.whole_frame()
    low64, iou64, low32, iou32, out64 = C.whole_reference(ref64, frame, boxes)
    bar = 4 * (low32.double() - low64).abs().max().item()
    assert out64.shape == (len(boxes), 1, 135, 240) and 0 < bar < 1e-3
    assert (out64.abs() <= bar).float().mean().item() <= 0.005 and 0.01 < (out64 > 0).float().mean().item() < 0.99
