"""CPU: the ABI of the recomputing DCN weight gradient (``sgv3d_deform_conv3x3_backward_weight_bf16`` and its host-only
``..._workspace_bytes``: header arity against the ctypes table, coverage, every rejection before any HIP call -- no GPU here) and
the float64 restatement of tests/dcn_grad_ref.py against a direct einsum and float64 autograd of the oracle."""
import os
import re

import pytest
import torch

import dcn_grad_ref as R
from oracle import torch_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes", "sgv3d_deform_conv3x3_backward_weight_bf16")


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


@pytest.mark.parametrize("name", NEW)
def test_header_arity_equals_ctypes_arity(name):
    from sgv3d_amd import _lib
    assert name in _lib.EXPORTED_SYMBOLS
    assert _header_arity(name) == len(_lib._PROTOS[name][1]), name
    assert getattr(_lib.load(), name) is not None


def test_workspace_bytes_is_host_only_and_knows_the_coverage():
    from sgv3d_amd import _lib
    f = _lib.load().sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes
    # (batch, h, w, channels, groups, out_per_group, split)
    assert f(2, 54, 96, 512, 4, 128, 1) == 9 * 512 * 128 * 4
    assert f(2, 54, 96, 512, 4, 128, 3) == 3 * 9 * 512 * 128 * 4
    assert f(2, 54, 96, 512, 4, 128, 0) % (9 * 512 * 128 * 4) == 0 and f(2, 54, 96, 512, 4, 128, 0) > 0
    assert f(3, 5, 5, 64, 2, 132, 0) == 9 * 264 * 32 * 4                     # 75 pixels: one range
    assert f(3, 5, 5, 64, 2, 132, 100) == 3 * 9 * 264 * 32 * 4               # never more ranges than 32-pixel steps
    for bad in ((1, 8, 8, 64, 4, 32, 0),         # 16 channels per group
                (1, 8, 8, 64, 2, 6, 0),          # opg % 4
                (1, 8, 8, 288, 9, 32, 0),        # 9 groups
                (1, 8, 8, 100, 3, 32, 0),        # channels % groups
                (0, 8, 8, 64, 2, 32, 0), (1, 0, 8, 64, 2, 32, 0), (1, 8, -1, 64, 2, 32, 0), (1, 8, 8, 64, 2, 0, 0),
                (1, 8, 8, 64, 2, 32, -1),
                (8, 1024, 1024, 64, 2, 32, 0)):  # x of 2 GiB
        assert f(*bad) == 0, bad
        assert b"deform_conv3x3_backward_weight_bf16_workspace_bytes" in _lib.load().sgv3d_last_error(), bad


# The pointers are never dereferenced: every case below is refused before a launch.
_GOOD = dict(sizes=(2, 9, 11, 128, 4, 32), x=0x10000, off=0x20000, off_ld=18, dy=0x30000, dw=0x40000, split=0, ws=0x50000, ws_bytes=1 << 30)


def _call(lib, **over):
    a = dict(_GOOD, **over)
    return lib.sgv3d_deform_conv3x3_backward_weight_bf16(*a['sizes'], a['x'], a['off'], a['off_ld'], a['dy'], a['dw'], a['split'], a['ws'],
                                                         a['ws_bytes'], None)


def test_argument_validation_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    need = lib.sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes(*_GOOD['sizes'], 0)
    assert need > 0
    bad = [dict(x=None), dict(off=None), dict(dy=None), dict(dw=None), dict(ws=None)]
    bad += [dict(sizes=(2, 9, 11, 64, 4, 32)), dict(sizes=(2, 9, 11, 128, 4, 30)), dict(sizes=(2, 9, 11, 288, 9, 32)),
            dict(sizes=(2, 9, 11, 100, 3, 32)), dict(sizes=(0, 9, 11, 128, 4, 32)), dict(sizes=(2, 9, 11, 128, 0, 32))]
    bad += [dict(off_ld=17), dict(off_ld=0)]
    bad += [dict(x=0x10004), dict(x=0x10008), dict(dy=0x30004), dict(ws=0x50008), dict(dw=0x40002), dict(off=0x20001)]
    bad += [dict(sizes=(8, 1024, 1024, 64, 2, 32)), dict(sizes=(1, 1024, 1024, 32, 1, 512))]        # x / dy of 2 GiB
    bad += [dict(split=-1)]
    for over in bad:
        rc = _call(lib, **over)
        msg = lib.sgv3d_last_error()
        assert rc == -1 and b"deform_conv3x3_backward_weight_bf16:" in msg, (over, rc, msg)
    rc = _call(lib, sizes=(2, 9, 11, 64, 4, 30))
    msg = lib.sgv3d_last_error()
    assert rc == -1 and b"cpg=16" in msg and b"opg=30" in msg, msg              # one message names both
    for short in (need - 1, 0):
        rc = _call(lib, ws_bytes=short)
        assert rc == -3 and b"workspace too small" in lib.sgv3d_last_error(), (short, rc)


def test_operator_refuses_cpu_tensors_and_uncovered_shapes():
    from sgv3d_amd import _lib, hip_ops, misc_grad
    assert misc_grad.deform_conv3x3_covers(512, 4, 512) and misc_grad.deform_conv3x3_covers(64, 2, 264)
    assert not misc_grad.deform_conv3x3_covers(64, 4, 64) and not misc_grad.deform_conv3x3_covers(128, 4, 120)
    assert not misc_grad.deform_conv3x3_covers(288, 9, 288) and not misc_grad.deform_conv3x3_covers(100, 3, 96)
    with pytest.raises(_lib.SGV3DError):
        misc_grad.deform_conv3x3(torch.zeros(1, 4, 4, 128), torch.zeros(1, 4, 4, 18), torch.zeros(128, 32, 3, 3), 4)
    saved, before = hip_ops.DCN_FUSED_TRAIN, hip_ops.switch_state()
    try:
        hip_ops.DCN_FUSED_TRAIN = not saved
        assert hip_ops.switch_state() != before                                   # the switch is part of switch_state()
    finally:
        hip_ops.DCN_FUSED_TRAIN = saved


@pytest.mark.parametrize("shape", [(2, 64, 5, 6, 2, 24), (1, 32, 4, 7, 1, 8)])
def test_restatement_dw_equals_einsum_and_autograd(shape):
    """(B, C, H, W, groups, cout): the rounded-operand dW against a direct einsum over the oracle's column tensor; the unrounded
    one against float64 autograd of the oracle's deform_conv3x3."""
    B, C, H, W, g, cout = shape
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, C, generator=gen)
    off = torch.randn(B, H, W, 18, generator=gen) * 1.5
    off[0, 0, 0] = 40.0
    off[-1, -1, -1] = -40.0
    w = torch.randn(cout, C // g, 3, 3, generator=gen)
    dy = torch.randn(B, H, W, cout, generator=gen)
    cpg, opg = C // g, cout // g
    col = TM.deform_im2col3x3(R.nchw(x.double()), R.nchw(off.double()))                   # [B, C, 9, H, W]
    cr = col.float().bfloat16().double()
    dr = R.nchw(dy).bfloat16().double()                                                     # [B, cout, H, W]
    direct = torch.stack([torch.einsum('bohw,bcthw->oct', dr[:, gi * opg:(gi + 1) * opg], cr[:, gi * cpg:(gi + 1) * cpg]) for gi in range(g)])
    direct = direct.reshape(cout, cpg, 3, 3)
    ref = R.backward(x, off, w, dy, g, rounded=True)
    assert (ref['dw'] - direct).abs().max() <= 1e-12 * direct.abs().max()
    assert (ref['dw'].abs() <= ref['dw_abs'] * (1 + 1e-12)).all()
    plain = R.backward(x, off, w, dy, g)
    assert (plain['dw'] - plain['dw_autograd']).abs().max() <= 1e-12 * plain['dw_autograd'].abs().max()
    assert plain['dx'].shape == x.shape and plain['doff'].shape == off.shape and float(plain['doff'].abs().max()) > 0
