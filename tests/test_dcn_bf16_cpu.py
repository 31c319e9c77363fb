"""CPU: the one-launch bf16 deformable convolution (csrc/dcn_fused_bf16.hip) is declared in include/sgv3d_hip.h and in the
ctypes table with the same arity, and refuses bad arguments before any HIP call (no GPU here)."""
import os
import re

from conftest import ROOT

NAMES = ("sgv3d_deform_conv3x3_forward_bf16", "sgv3d_deform_conv3x3_bf16_pack_weight", "sgv3d_deform_conv3x3_bf16_weight_bytes")


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in sgv3d_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_symbols_declared_with_matching_arity():
    from sgv3d_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        params = _header_params(name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(params), (name, params)
    assert len(_header_params(NAMES[0])) == 16


def test_weight_bytes_is_host_only():
    from sgv3d_amd import _lib
    lib = _lib.load()
    # [groups][8 blocks of 16 channels per 128][9 * cpg / 32 k-steps][64 lanes][8] bf16
    assert lib.sgv3d_deform_conv3x3_bf16_weight_bytes(512, 4, 128) == 4 * 8 * 36 * 1024
    assert lib.sgv3d_deform_conv3x3_bf16_weight_bytes(64, 2, 132) == 2 * 16 * 9 * 1024
    assert lib.sgv3d_deform_conv3x3_bf16_weight_bytes(64, 4, 16) == 0            # 16 channels per group
    assert lib.sgv3d_deform_conv3x3_bf16_weight_bytes(512, 4, 126) == 0          # outputs per group % 4
    assert lib.sgv3d_deform_conv3x3_bf16_weight_bytes(512 * 9, 9, 128) == 0      # more than 8 groups
    assert lib.sgv3d_deform_conv3x3_bf16_weight_bytes(510, 4, 128) == 0          # channels % groups


def test_argument_validation_without_gpu():
    """Bad arguments are rejected before any HIP call is made: the pointers below are never dereferenced."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    fwd = lib.sgv3d_deform_conv3x3_forward_bf16
    p = 0x1000                                                   # 16-byte aligned, never touched

    def call(batch=1, h=8, w=8, channels=128, groups=4, opg=32, x=p, x_bf16=1, off=p, off_ld=18, wp=p, y=p, y_bf16=0, y_ld=128,
             y_coff=0):
        return fwd(batch, h, w, channels, groups, opg, x, x_bf16, off, off_ld, wp, y, y_bf16, y_ld, y_coff, None)

    for null in ("x", "off", "wp", "y"):
        assert call(**{null: None}) == -1 and b"null pointer" in lib.sgv3d_last_error(), null
    assert call(channels=130) == -1 and b"bad shape" in lib.sgv3d_last_error()                  # channels % groups
    assert call(off_ld=16) == -1 and b"bad shape" in lib.sgv3d_last_error()
    assert call(channels=9 * 32, groups=9) == -1 and b"bad shape" in lib.sgv3d_last_error()    # groups > 8
    assert call(batch=0) == -1 and b"bad shape" in lib.sgv3d_last_error()
    assert call(channels=64) == -1 and b"cpg=16 opg=32" in lib.sgv3d_last_error()               # 16 channels per group (one message
    assert call(opg=30, y_ld=120) == -1 and b"cpg=32 opg=30" in lib.sgv3d_last_error()          #  names every geometry condition)
    assert call(y_ld=124) == -1                                                                  # narrower than the channels written
    assert call(y_ld=136, y_coff=6) == -1                                                        # offset % 4
    assert call(x=p + 8) == -1 and b"aligned" in lib.sgv3d_last_error()
    assert call(batch=4096, h=1024, w=1024) == -1 and b"2 GiB" in lib.sgv3d_last_error()
    pack = lib.sgv3d_deform_conv3x3_bf16_pack_weight
    assert pack(None, 128, 4, 32, p, None) == -1 and b"null pointer" in lib.sgv3d_last_error()
    assert pack(p, 64, 4, 32, p, None) == -1 and b"channels per group" in lib.sgv3d_last_error()
