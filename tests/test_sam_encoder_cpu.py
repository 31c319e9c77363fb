"""CPU: the SAM ViT encoder without a GPU -- the float64 restatement (tests/vit_ref.py) against the reference's recorded
outputs, the new C ABI entries (header against ctypes, every rejection before any HIP call), the module's parameter
names against the reference's, and the module's own refusals."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import vit_ref as V
from conftest import GOLDEN, ROOT

ENTRIES = ("sgv3d_vit_attention", "sgv3d_layernorm", "sgv3d_gelu", "sgv3d_vit_preprocess", "sgv3d_resize_bilinear")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "sam_encoder.npz"))


@pytest.fixture(scope="module")
def restated(fixture):
    """The restatement's float64 run on the fixture's weights and input, computed once: (output, block outputs)."""
    wts = {k[2:]: torch.from_numpy(fixture[k]) for k in fixture.files if k.startswith('w/')}
    blocks = []
    out = V.encoder_forward(wts, V.FIXTURE_CFG, torch.from_numpy(fixture['input']).double(), blocks)
    return out, blocks


def test_restatement_matches_the_reference_output(fixture, restated):
    assert tuple(restated[0].shape) == (2, 32, 13, 24)
    assert float((restated[0] - torch.from_numpy(fixture['out'])).abs().max()) <= 1e-12


def test_restatement_matches_every_block(fixture, restated):
    assert len(restated[1]) == 2
    for i, b in enumerate(restated[1]):
        assert float((b - torch.from_numpy(fixture[f'block{i}'])).abs().max()) <= 1e-12


def test_fixture_sees_the_three_misreadings(fixture):
    """Padding keys masked, padding tokens zero, scaled q in the rel-pos terms: each is far outside any bar."""
    wts = {k[2:]: torch.from_numpy(fixture[k]) for k in fixture.files if k.startswith('w/')}
    x = torch.from_numpy(fixture['input']).double()
    want = torch.from_numpy(fixture['out'])
    for kw in (dict(pad_keys='masked'), dict(pad_keys='zero'), dict(rel_uses_scaled_q=True)):
        assert float((V.encoder_forward(wts, V.FIXTURE_CFG, x, **kw) - want).abs().max()) > 1e-2, kw


# ------------------------------------------------------------------------------------------------
def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in sgv3d_hip.h"
        protos[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    return text, protos


def _ctype_of(decl):
    if "*" in decl:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}[decl.rsplit(" ", 1)[0]]


def test_header_matches_ctypes():
    from sgv3d_amd import _lib
    text, protos = _header_prototypes()
    for name, args in protos.items():
        res, argtypes = _lib._PROTOS[name]
        assert res is ctypes.c_int
        want = [_ctype_of(a) for a in args]
        got = [ctypes.c_void_p if (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t for t in argtypes]
        assert got == want, f"{name}: ctypes {got} against the header's {args}"
    body = text[text.index("typedef struct sgv3d_vit_attn_desc"):text.index("} sgv3d_vit_attn_desc;")]
    fields = []
    for decl in re.findall(r"int\s+([^;]+);", body):
        fields += [f.strip() for f in decl.split(",")]
    assert fields == [f[0] for f in _lib.VitAttnDesc._fields_]
    assert ctypes.sizeof(_lib.VitAttnDesc) == 4 * len(fields)


A = 4096          # a non-null, 16-byte aligned address: every call below is refused before it is looked at


def _rejected(lib, rc, word):
    msg = lib.sgv3d_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_attention_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.VitAttnDesc
    call = lambda d, qkv=A, pad=A, rh=A, rw=A, out=A: lib.sgv3d_vit_attention(ctypes.byref(d) if d else None, qkv, pad, rh, rw, out, None)
    _rejected(lib, call(None), "null descriptor")
    for hd in (16, 48, 96, 128):
        _rejected(lib, call(D(1, 8, 8, 2, hd, 8, 8)), "head_dim")
    for i in range(7):                         # a zero in every field
        v = [1, 8, 8, 2, 32, 8, 8]
        v[i] = 0
        _rejected(lib, call(D(*v)), "zero or negative dimension")
    _rejected(lib, call(D(1, 8, 8, 1, 33, 8, 8)), "is not a multiple of 4")
    _rejected(lib, call(D(1, 8, 8, 3, 30, 8, 8)), "is not a multiple of 4")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 129, 8)), "exceeds 128")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 129)), "exceeds 128")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 8), rh=None), "given together")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 8), rw=None), "given together")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 8), qkv=None), "null qkv or out")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 8), out=None), "null qkv or out")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 8), qkv=A + 4), "16-byte aligned")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 8), pad=A + 8), "16-byte aligned")


def test_small_kernel_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float
    _rejected(lib, lib.sgv3d_layernorm(0, 8, A, A, A, f(1e-6), A, None), "non-positive")
    _rejected(lib, lib.sgv3d_layernorm(4, 0, A, A, A, f(1e-6), A, None), "non-positive")
    _rejected(lib, lib.sgv3d_layernorm(4, 6, A, A, A, f(1e-6), A, None), "multiple of 4")
    _rejected(lib, lib.sgv3d_layernorm(4, 8, None, A, A, f(1e-6), A, None), "null pointer")
    _rejected(lib, lib.sgv3d_layernorm(4, 8, A, None, A, f(1e-6), A, None), "null pointer")
    _rejected(lib, lib.sgv3d_layernorm(4, 8, A, A, None, f(1e-6), A, None), "null pointer")
    _rejected(lib, lib.sgv3d_layernorm(4, 8, A, A, A, f(1e-6), None, None), "null pointer")
    _rejected(lib, lib.sgv3d_layernorm(4, 8, A, A, A, f(-1.0), A, None), "negative eps")
    _rejected(lib, lib.sgv3d_layernorm(4, 8, A + 4, A, A, f(1e-6), A, None), "16-byte aligned")

    _rejected(lib, lib.sgv3d_gelu(0, A, A, None), "non-positive")
    _rejected(lib, lib.sgv3d_gelu(8, None, A, None), "null pointer")
    _rejected(lib, lib.sgv3d_gelu(8, A, None, None), "null pointer")
    _rejected(lib, lib.sgv3d_gelu(8, A, A + 4, None), "16-byte aligned")

    _rejected(lib, lib.sgv3d_vit_preprocess(0, 54, 96, A, A, A, 96, A, None), "non-positive")
    _rejected(lib, lib.sgv3d_vit_preprocess(1, 54, 96, A, A, A, 0, A, None), "non-positive")
    _rejected(lib, lib.sgv3d_vit_preprocess(1, 54, 90, A, A, A, 96, A, None), "long side")
    _rejected(lib, lib.sgv3d_vit_preprocess(1, 54, 100, A, A, A, 96, A, None), "long side")
    for i in (3, 4, 5, 7):
        args = [1, 54, 96, A, A, A, 96, A, None]
        args[i] = None
        _rejected(lib, lib.sgv3d_vit_preprocess(*args), "null pointer")
    _rejected(lib, lib.sgv3d_vit_preprocess(1, 54, 96, A, A, A, 96, A + 4, None), "16-byte aligned")

    for i in range(8):
        args = [1, 12, 12, 8, 9, 16, 13, 24, A, A, None]
        args[i] = 0
        _rejected(lib, lib.sgv3d_resize_bilinear(*args), "non-positive")
    _rejected(lib, lib.sgv3d_resize_bilinear(1, 12, 12, 6, 9, 16, 13, 24, A, A, None), "multiple of 4")
    _rejected(lib, lib.sgv3d_resize_bilinear(1, 12, 12, 8, 9, 16, 13, 24, None, A, None), "null pointer")
    _rejected(lib, lib.sgv3d_resize_bilinear(1, 12, 12, 8, 9, 16, 13, 24, A, None, None), "null pointer")
    _rejected(lib, lib.sgv3d_resize_bilinear(1, 12, 12, 8, 9, 16, 13, 24, A, A + 8, None), "16-byte aligned")


def test_key_row_without_integer_division():
    """The attention kernel splits a window slot t into (kh, kw) as kh = int((float(t) + 0.5f) * (1.0f / win_w)): the same
    float32 expression agrees with t // win_w for every window width up to 128 and every slot of a 128-row window."""
    for w in range(1, 129):
        inv = np.float32(1.0) / np.float32(w)
        t = np.arange(128 * w, dtype=np.int64)
        kh = ((t.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
        assert np.array_equal(kh, t // w), w


# ------------------------------------------------------------------------------------------------
def test_vit_b_parameter_names_and_shapes(fixture):
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b
    model = build_sam_vit_b((864, 1536), 16)
    names = [k for k, _ in model.named_parameters()]
    shapes = [list(v.shape) for _, v in model.named_parameters()]
    assert names == json.loads(str(fixture['vit_b_names']))
    assert shapes == json.loads(str(fixture['vit_b_shapes']))
    assert set(model.state_dict()) == set(names)            # pixel_mean / pixel_std are not persistent, as in the reference
    assert model.input_size == (36, 64) and model.out_dim == (54, 96)


def test_vit_l_and_vit_h_constructor_numbers():
    from sgv3d_amd.layers.backbones import sam_encoder as S
    seen = {}
    orig = S.ImageEncoderViT
    S.ImageEncoderViT = lambda **kw: seen.update(kw)
    try:
        S.build_sam_vit_l((864, 1536), 16)
        assert (seen['embed_dim'], seen['depth'], seen['num_heads'], seen['global_attn_indexes']) == (1024, 24, 16, [5, 11, 17, 23])
        S.build_sam_vit_h((864, 1536), 16)
        assert (seen['embed_dim'], seen['depth'], seen['num_heads'], seen['global_attn_indexes']) == (1280, 32, 16, [7, 15, 23, 31])
        assert seen['window_size'] == 14 and seen['img_size'] == 1024 and seen['patch_size'] == 16 and seen['use_rel_pos']
    finally:
        S.ImageEncoderViT = orig


def test_get_image_encoder_strips_the_prefix():
    from sgv3d_amd.layers.backbones.sam_encoder import get_image_encoder
    sd = {"image_encoder.pos_embed": 1, "image_encoder.blocks.0.attn.qkv.weight": 2, "prompt_encoder.pe": 3, "mask_decoder.x": 4}
    assert get_image_encoder(sd) == {"pos_embed": 1, "blocks.0.attn.qkv.weight": 2}


def test_fixture_weights_load_by_name(fixture):
    from functools import partial
    from sgv3d_amd.layers.backbones.sam_encoder import ImageEncoderViT
    cfg = V.FIXTURE_CFG
    model = ImageEncoderViT(img_size=cfg['img_size'], patch_size=cfg['patch_size'], embed_dim=cfg['embed_dim'], depth=cfg['depth'],
                            num_heads=cfg['num_heads'], out_chans=cfg['out_chans'], window_size=cfg['window_size'],
                            global_attn_indexes=cfg['global_attn_indexes'], use_rel_pos=True,
                            norm_layer=partial(torch.nn.LayerNorm, eps=cfg['eps']), final_dim=cfg['final_dim'],
                            downsample_factor=cfg['downsample_factor'])
    wts = {"image_encoder." + k[2:]: torch.from_numpy(fixture[k]) for k in fixture.files if k.startswith('w/')}
    from sgv3d_amd.layers.backbones.sam_encoder import get_image_encoder
    model.load_state_dict(get_image_encoder(wts))           # strict: every name and shape
    assert model.blocks[0].window_size == 5 and model.blocks[1].window_size == 0
    assert tuple(model.blocks[0].attn.rel_pos_h.shape) == (9, 32) and tuple(model.blocks[1].attn.rel_pos_w.shape) == (23, 32)


def test_module_refusals():
    from sgv3d_amd._lib import SGV3DError
    from sgv3d_amd.layers.backbones.sam_encoder import Attention, ImageEncoderViT
    attn = Attention(64, num_heads=2, use_rel_pos=True, input_size=(5, 5))
    with pytest.raises(SGV3DError, match="rel_pos_h has 9 rows, a 7 x 7 window needs 13"):
        attn(torch.zeros(1, 7, 7, 64))
    with pytest.raises(SGV3DError, match="rel_pos_w has 9 rows"):
        attn(torch.zeros(1, 5, 5, 64), window=(5, 6))
    with pytest.raises(SGV3DError, match="inference only: the input requires grad"):
        attn(torch.zeros(1, 5, 5, 64, requires_grad=True))
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        attn(torch.zeros(1, 5, 5, 64))
    enc = ImageEncoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, out_chans=8)
    with pytest.raises(SGV3DError, match="inference only: the input requires grad"):
        enc(torch.zeros(1, 3, 32, 32, requires_grad=True))
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        enc(torch.zeros(1, 3, 32, 32))
