"""CPU: the SAM ViT encoder's bf16 mode without a GPU -- the three C ABI entries of csrc/vit_bf16.hip (header against ctypes,
every rejection by name before any HIP call), the coverage rule, and the module's refusals."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("sgv3d_vit_attention_bf16", "sgv3d_layernorm_bf16out", "sgv3d_gelu_bf16")
A = 4096          # a non-null, 16-byte aligned address: every call below is refused before it is looked at


def _ctype_of(decl):
    if "*" in decl:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}[decl.rsplit(" ", 1)[0]]


def test_header_matches_ctypes():
    from sgv3d_amd import _lib
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in sgv3d_hip.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        res, argtypes = _lib._PROTOS[name]
        assert res is ctypes.c_int
        got = [ctypes.c_void_p if (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t for t in argtypes]
        assert got == [_ctype_of(a) for a in args], f"{name}: ctypes {got} against the header's {args}"
        assert name in _lib.EXPORTED_SYMBOLS
    # bf16 tensors are void *, the parameters stay float *
    m = re.search(r"sgv3d_vit_attention_bf16\s*\(([^)]*)\)", text).group(1)
    assert "const void *qkv" in m and "void *out" in m and "const float *pad_qkv" in m and "const float *rel_pos_h" in m


def _rejected(lib, rc, word):
    msg = lib.sgv3d_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_attention_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.VitAttnDesc
    call = lambda d, qkv=A, pad=A, rh=A, rw=A, out=A: lib.sgv3d_vit_attention_bf16(ctypes.byref(d) if d else None, qkv, pad, rh, rw, out,
                                                                                    None)
    ok = (1, 8, 8, 2, 32, 8, 8)
    _rejected(lib, call(None), "null descriptor")
    for hd in (16, 48, 96, 128):
        _rejected(lib, call(D(1, 8, 8, 2, hd, 8, 8)), "head_dim")
    for i in range(7):                         # a zero in every field
        v = list(ok)
        v[i] = 0
        _rejected(lib, call(D(*v)), "zero or negative dimension")
    _rejected(lib, call(D(1, 8, 8, 1, 33, 8, 8)), "is not a multiple of 8")
    _rejected(lib, call(D(1, 8, 8, 3, 30, 8, 8)), "is not a multiple of 8")
    _rejected(lib, call(D(1, 8, 8, 1, 36, 8, 8)), "is not a multiple of 8")       # a multiple of 4: the f32 entry's rule is not enough
    _rejected(lib, call(D(1, 8, 8, 2, 32, 129, 8)), "exceeds 128")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 129)), "exceeds 128")
    _rejected(lib, call(D(*ok), rh=None), "given together")
    _rejected(lib, call(D(*ok), rw=None), "given together")
    _rejected(lib, call(D(*ok), qkv=None), "null qkv or out")
    _rejected(lib, call(D(*ok), out=None), "null qkv or out")
    for kw in (dict(qkv=A + 2), dict(qkv=A + 8), dict(out=A + 8), dict(pad=A + 4), dict(rh=A + 4), dict(rw=A + 8)):
        _rejected(lib, call(D(*ok), **kw), "16-byte aligned")
    _rejected(lib, call(D(1, 8, 8, 1 << 18, 80, 8, 8)), "too large")


def test_small_kernel_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float
    ln = lib.sgv3d_layernorm_bf16out
    _rejected(lib, ln(0, 8, A, A, A, f(1e-6), A, None), "non-positive")
    _rejected(lib, ln(4, 0, A, A, A, f(1e-6), A, None), "non-positive")
    _rejected(lib, ln(4, 4, A, A, A, f(1e-6), A, None), "multiple of 8")
    _rejected(lib, ln(4, 36, A, A, A, f(1e-6), A, None), "multiple of 8")
    for i in (2, 3, 4, 6):
        args = [4, 8, A, A, A, f(1e-6), A, None]
        args[i] = None
        _rejected(lib, ln(*args), "null pointer")
    _rejected(lib, ln(4, 8, A, A, A, f(-1.0), A, None), "negative eps")
    for i in (2, 3, 4, 6):
        args = [4, 8, A, A, A, f(1e-6), A, None]
        args[i] = A + 8
        _rejected(lib, ln(*args), "16-byte aligned")

    _rejected(lib, lib.sgv3d_gelu_bf16(0, A, A, None), "non-positive")
    _rejected(lib, lib.sgv3d_gelu_bf16(-3, A, A, None), "non-positive")
    _rejected(lib, lib.sgv3d_gelu_bf16(8, None, A, None), "null pointer")
    _rejected(lib, lib.sgv3d_gelu_bf16(8, A, None, None), "null pointer")
    _rejected(lib, lib.sgv3d_gelu_bf16(8, A + 2, A, None), "16-byte aligned")
    _rejected(lib, lib.sgv3d_gelu_bf16(8, A, A + 8, None), "16-byte aligned")


def test_vit_bf16_covers():
    from sgv3d_amd.hip_ops import vit_bf16_covers
    assert vit_bf16_covers(768, 12) and vit_bf16_covers(1024, 16) and vit_bf16_covers(1280, 16)      # ViT-B / L / H
    assert vit_bf16_covers(64, 2) and vit_bf16_covers(64, 2, 256)                                   # the fixture model
    assert not vit_bf16_covers(768, 8)              # head_dim 96
    assert not vit_bf16_covers(96, 2)               # head_dim 48
    assert not vit_bf16_covers(100, 3)              # not divisible
    assert not vit_bf16_covers(768, 12, 3076)       # mlp_dim % 8
    assert not vit_bf16_covers(768, 12, 0) and not vit_bf16_covers(0, 12) and not vit_bf16_covers(768, 0)


@pytest.fixture
def switches():
    from sgv3d_amd import hip_ops
    saved = (hip_ops.VIT_BF16, hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3)
    yield hip_ops
    hip_ops.VIT_BF16, hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3 = saved


def test_switch_is_off_by_default_and_needs_bf16_mode(switches):
    """Without MFMA_BF16, or with the f32x3 split, the switch changes nothing: the Block takes its f32-tensor path."""
    from sgv3d_amd.layers.backbones.sam_encoder import Block
    hip_ops = switches
    if not os.environ.get("SGV3D_VIT_BF16"):
        assert hip_ops.VIT_BF16 is False
    blk = Block(64, 2, use_rel_pos=True, window_size=5, input_size=(12, 12))
    odd = Block(96, 2, input_size=(12, 12))           # head_dim 48: not covered
    for vit, bf16, x3, want in ((False, True, False, False), (True, False, False, False), (True, True, True, False),
                                (True, True, "auto", False), (True, True, False, True)):
        hip_ops.VIT_BF16, hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3 = vit, bf16, x3
        assert hip_ops.vit_bf16_active(64, 2, 256) is want
        assert blk.bf16_mode() is want
        assert odd.bf16_mode() is False
    hip_ops.VIT_BF16 = False
    off = hip_ops.switch_state()
    hip_ops.VIT_BF16 = True
    assert hip_ops.switch_state() != off


def test_module_refusals_in_bf16_mode(switches):
    from sgv3d_amd._lib import SGV3DError
    from sgv3d_amd.layers.backbones.common import MLPBlock
    from sgv3d_amd.layers.backbones.sam_encoder import Attention, Block, ImageEncoderViT
    hip_ops = switches
    hip_ops.VIT_BF16, hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3 = True, True, False
    blk = Block(64, 2, use_rel_pos=True, window_size=5, input_size=(12, 12))
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        blk(torch.zeros(1, 5, 5, 64))
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        Attention(64, num_heads=2)(torch.zeros(1, 5, 5, 64, dtype=torch.bfloat16))
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        MLPBlock(64, 256)(torch.zeros(1, 5, 5, 64, dtype=torch.bfloat16))
    enc = ImageEncoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, out_chans=8)
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        enc(torch.zeros(1, 3, 32, 32))
    with pytest.raises(SGV3DError, match="inference only: the input requires grad"):
        enc(torch.zeros(1, 3, 32, 32, requires_grad=True))
