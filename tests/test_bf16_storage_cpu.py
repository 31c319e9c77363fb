"""CPU: the bf16-activation-storage entries (bf16 BatchNorm, bf16-tensor weight gradients) -- header against ctypes, every argument
rejection (they all happen before any HIP call), the coverage rule of the switch, and the float64 restatements that the GPU tests use
against torch's float64 autograd."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bf16_storage_ref as R
from conftest import ROOT

NEW = ("sgv3d_batchnorm_train_forward_bf16", "sgv3d_batchnorm_train_backward_bf16", "sgv3d_batchnorm_relu_train_backward_from_x_bf16",
       "sgv3d_conv2d_backward_weight_bf16_tensors", "sgv3d_conv2d_backward_weight_bf16_tensors_workspace_bytes",
       "sgv3d_conv2d_backward_weight_bf16_alltaps_tensors", "sgv3d_conv2d_backward_weight_bf16_alltaps_tensors_workspace_bytes")


def _declared_arity(name):
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in sgv3d_hip.h"
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


@pytest.mark.parametrize("name", NEW)
def test_header_and_ctypes_prototypes_agree(name):
    from sgv3d_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    assert len(_lib._PROTOS[name][1]) == _declared_arity(name)
    # the f32 twins have the same shape of call
    twin = name.replace("_tensors", "").replace("_from_x_bf16", "_from_x").replace("_forward_bf16", "_forward").replace("_backward_bf16", "_backward")
    if "alltaps" not in name or not name.endswith("workspace_bytes"):       # (the f32 all-taps workspace function also takes n)
        assert len(_lib._PROTOS[name][1]) == len(_lib._PROTOS[twin][1])


def _err(lib):
    return lib.sgv3d_last_error().decode()


A = 0x10000            # a 16-byte aligned address that is never dereferenced: every call below is refused before any HIP call


def _fwd(lib, pixels=64, C=64, x=A, res=None, y=A, mean=A, invstd=A, ws=A, nws=None):
    nws = lib.sgv3d_batchnorm_workspace_bytes(C if C > 0 else 8) if nws is None else nws
    return lib.sgv3d_batchnorm_train_forward_bf16(pixels, C, x, res, A, A, None, None, 0.1, 1e-5, 1, y, mean, invstd, ws, nws, None)


def _bwd(lib, pixels=64, C=64, x=A, y=A, dy=A, relu=1, dx=A, dres=None, dg=A, db=A, mean=A, invstd=A, ws=A, nws=None, gamma=A):
    nws = lib.sgv3d_batchnorm_workspace_bytes(C if C > 0 else 8) if nws is None else nws
    return lib.sgv3d_batchnorm_train_backward_bf16(pixels, C, x, y, dy, gamma, mean, invstd, relu, dx, dres, dg, db, ws, nws, None)


def _bwx(lib, pixels=64, C=64, x=A, dy=A, dx=A, dg=A, db=A, mean=A, invstd=A, ws=A, nws=None, gamma=A, beta=A):
    nws = lib.sgv3d_batchnorm_workspace_bytes(C if C > 0 else 8) if nws is None else nws
    return lib.sgv3d_batchnorm_relu_train_backward_from_x_bf16(pixels, C, x, dy, gamma, beta, mean, invstd, dx, dg, db, ws, nws, None)


def test_batchnorm_bf16_rejects_bad_arguments_without_a_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    for call in (_fwd, _bwd, _bwx):
        for C in (4, 12, 36, 0, -8):                                    # a 16-byte load is 8 channels
            assert call(lib, C=C) == -1, (call.__name__, C)
            assert "channels" in _err(lib)
        assert call(lib, pixels=0) == -1 and "pixels" in _err(lib)
        assert call(lib, nws=lib.sgv3d_batchnorm_workspace_bytes(64) - 1) == -1 and "workspace too small" in _err(lib)
        assert call(lib, ws=None) == -1 and "null" in _err(lib)
        assert call(lib, ws=A + 8) == -1 and "aligned" in _err(lib)
        assert call(lib, x=None) == -1 and "null" in _err(lib)
        assert call(lib, x=A + 2) == -1 and "aligned" in _err(lib)
        assert call(lib, mean=None) == -1 and "null" in _err(lib)
        assert call(lib, invstd=None) == -1 and "null" in _err(lib)
    assert _fwd(lib, y=None) == -1 and "null" in _err(lib)
    assert _fwd(lib, y=A + 4) == -1 and "aligned" in _err(lib)
    assert _fwd(lib, res=A + 8) == -1 and "aligned" in _err(lib)
    for call in (_bwd, _bwx):
        for k in ("dy", "dx", "dg", "db"):
            assert call(lib, **{k: None}) == -1 and "null" in _err(lib), (call.__name__, k)
            assert call(lib, **{k: A + 8}) == -1 and "aligned" in _err(lib), (call.__name__, k)
        assert call(lib, gamma=A + 4) == -1 and "aligned" in _err(lib)
        assert call(lib, mean=A + 4) == -1 and "aligned" in _err(lib)
    assert _bwd(lib, y=None, relu=1) == -1 and "ReLU mask" in _err(lib)
    assert _bwd(lib, y=A + 8) == -1 and "aligned" in _err(lib)
    assert _bwd(lib, dres=A + 8) == -1 and "aligned" in _err(lib)
    assert _bwx(lib, beta=A + 4) == -1 and "aligned" in _err(lib)


def _desc(_lib, cin=72, cout=40, k=3, stride=1, pad=1, dil=1, x_ld=None, y_ld=None, x_coff=0, y_coff=0, tile=0, hw=(12, 20)):
    d = _lib.ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin, d.cout = 2, hw[0], hw[1], cin, cout
    d.out_h = (hw[0] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    d.out_w = (hw[1] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    d.kh, d.kw, d.stride, d.pad, d.dil = k, k, stride, pad, dil
    d.x_ld, d.x_coff, d.y_ld, d.y_coff = (x_ld or cin + x_coff), x_coff, (y_ld or cout + y_coff), y_coff
    d.tile = tile
    return d


def test_weight_gradient_bf16_tensors_rejects_bad_arguments_without_a_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    per_tap = (lib.sgv3d_conv2d_backward_weight_bf16_tensors, lib.sgv3d_conv2d_backward_weight_bf16_tensors_workspace_bytes)
    alltaps = (lib.sgv3d_conv2d_backward_weight_bf16_alltaps_tensors, lib.sgv3d_conv2d_backward_weight_bf16_alltaps_tensors_workspace_bytes)
    for launch, wsb in (per_tap, alltaps):
        good = _desc(_lib)
        n = wsb(ctypes.byref(good), 3)
        assert n > 0
        # multiples of 8 for strides and offsets (the layout contract of the bf16 maps); the f32-tensor entries take multiples of 4
        for kw in (dict(x_ld=76), dict(y_ld=44), dict(x_coff=4, x_ld=80), dict(y_coff=4, y_ld=48)):
            bad = _desc(_lib, **kw)
            assert wsb(ctypes.byref(bad), 3) == 0, kw
            assert launch(ctypes.byref(bad), A, A, A, 3, A, 1 << 30, None) == -1 and "multiples of 8" in _err(lib), kw
        assert launch(ctypes.byref(_desc(_lib, cin=70, x_ld=72)), A, A, A, 3, A, 1 << 30, None) == -1 and "multiples of 4" in _err(lib)
        assert launch(None, A, A, A, 3, A, 1 << 30, None) == -1 and "null descriptor" in _err(lib)
        for args in ((None, A, A), (A, None, A), (A, A, None)):
            assert launch(ctypes.byref(good), *args, 3, A, n, None) == -1 and "null" in _err(lib)
        assert launch(ctypes.byref(good), A + 8, A, A, 3, A, n, None) == -1 and "aligned" in _err(lib)
        assert launch(ctypes.byref(good), A, A + 8, A, 3, A, n, None) == -1 and "aligned" in _err(lib)
        assert launch(ctypes.byref(good), A, A, A, 3, A, n - 1, None) == -1 and "workspace too small" in _err(lib)
        assert launch(ctypes.byref(good), A, A, A, 3, None, n, None) == -1
    # the per-tap form takes tiles 0, 1 and 4 only; the all-taps form 3x3 / stride 1 only
    assert per_tap[0](ctypes.byref(_desc(_lib, tile=2)), A, A, A, 3, A, 1 << 30, None) == -1 and "tile must be" in _err(lib)
    assert alltaps[0](ctypes.byref(_desc(_lib, stride=2)), A, A, A, 1, A, 1 << 30, None) == -1 and "3x3 / stride 1" in _err(lib)
    assert alltaps[1](ctypes.byref(_desc(_lib, k=1, pad=0)), 1) == 0
    # same workspace as the f32-tensor entries (same split, same partial layout)
    good = _desc(_lib)
    for sp in (0, 1, 3):
        assert per_tap[1](ctypes.byref(good), sp) == lib.sgv3d_conv2d_backward_weight_bf16_workspace_bytes(ctypes.byref(good), sp)
        assert alltaps[1](ctypes.byref(good), sp) == lib.sgv3d_conv2d_backward_weight_bf16_alltaps_workspace_bytes(ctypes.byref(good), 1, sp)


@pytest.fixture
def switches():
    from sgv3d_amd import hip_ops
    names = ("TRAIN_BF16_STORAGE", "MFMA_BF16", "MFMA_F32X3", "TRAIN_BF16_WGRAD", "BF16_ACTIVATIONS")
    saved = {n: getattr(hip_ops, n) for n in names}
    yield hip_ops
    for n, v in saved.items():
        setattr(hip_ops, n, v)


def test_switch_is_off_by_default_and_part_of_the_switch_state(switches):
    hip_ops = switches
    if not os.environ.get("SGV3D_TRAIN_BF16_STORAGE"):
        assert hip_ops.TRAIN_BF16_STORAGE is False
    hip_ops.TRAIN_BF16_STORAGE = False
    off = hip_ops.switch_state()
    hip_ops.TRAIN_BF16_STORAGE = True
    assert hip_ops.switch_state() != off


def test_covers_rule_on_the_shipped_configs_and_a_36_channel_stage(switches):
    from sgv3d_amd import synthetic, train_forward
    from sgv3d_amd.layers import blocks
    hip_ops = switches
    hip_ops.TRAIN_BF16_STORAGE, hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.TRAIN_BF16_WGRAD = True, True, False, True
    nets = {}
    for name, conf in (("r50", synthetic.r50_256_conf), ("r101", synthetic.bsm_r101_256_conf), ("r18", synthetic.small_conf)):
        bconf, _ = conf()
        cfg = dict(bconf['img_backbone_conf'])
        cfg.pop('type', None)
        cfg.pop('init_cfg', None)
        nets[name] = blocks.ResNet(**cfg)
        assert train_forward.resnet_storage_covers(nets[name]), name
    odd = blocks.ResNet(depth=18, base_channels=36, stem_channels=64, out_indices=(0, 1, 2, 3))         # 36-channel first stage
    assert not train_forward.resnet_storage_covers(odd)
    assert hip_ops.train_bf16_storage_covers([64, 72, 256]) and not hip_ops.train_bf16_storage_covers([64, 36]) and not hip_ops.train_bf16_storage_covers([])
    # an 8-channel stage: the bf16 weight-gradient kernels need at least 16 channels on both sides -> the f32 path, silently
    assert hip_ops.train_bf16_storage_covers([16, 24]) and not hip_ops.train_bf16_storage_covers([64, 8])
    assert not train_forward.resnet_storage_covers(blocks.ResNet(depth=18, base_channels=8, stem_channels=8, out_indices=(0, 1, 2, 3)))
    # every condition of the switch
    r = nets["r50"]
    for name, value in (("TRAIN_BF16_STORAGE", False), ("MFMA_BF16", False), ("MFMA_F32X3", True), ("MFMA_F32X3", "auto"), ("TRAIN_BF16_WGRAD", False)):
        old = getattr(hip_ops, name)
        setattr(hip_ops, name, value)
        assert not train_forward.resnet_storage_covers(r), (name, value)
        setattr(hip_ops, name, old)
    assert train_forward.resnet_storage_covers(r)


@pytest.mark.parametrize("use_res,relu,affine", [(False, True, True), (True, True, True), (True, False, True), (False, False, False)])
def test_float64_batchnorm_restatement_is_torch_autograd(use_res, relu, affine):
    g = torch.Generator().manual_seed(3)
    P, C = 45, 16
    x = (torch.randn(P, C, generator=g, dtype=torch.float64) * 0.7 + 0.2).requires_grad_(True)
    res = torch.randn(P, C, generator=g, dtype=torch.float64).requires_grad_(True) if use_res else None
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True) if affine else None
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True) if affine else None
    dy = torch.randn(P, C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.batch_norm(x.t().contiguous()[None, :, :, None], rm, rv, gamma, beta, True, 0.1, 1e-5)[0, :, :, 0].t()      # (NCHW, contiguous)
    if use_res:
        y = y + res
    if relu:
        y = F.relu(y)
    y.backward(dy)
    got = R.bn_act(x.detach(), None if res is None else res.detach(), None if gamma is None else gamma.detach(),
                   None if beta is None else beta.detach(), 1e-5, relu, dy)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-12)
    close(got['y'], y.detach())
    close(got['dx'], x.grad)
    if use_res:
        close(got['dres'], res.grad)
    if affine:
        close(got['dgamma'], gamma.grad)
        close(got['dbeta'], beta.grad)
    want_rm, want_rv = R.running((rm0, rv0), got['mean'], got['var'], P, 0.1)
    close(want_rm, rm)
    close(want_rv, rv)


@pytest.mark.parametrize("k,stride,pad,dil", [(1, 1, 0, 1), (3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2), (1, 2, 0, 1)])
def test_float64_weight_gradient_einsum_is_torch_autograd(k, stride, pad, dil):
    g = torch.Generator().manual_seed(k + stride)
    x = torch.randn(2, 7, 9, 5, generator=g, dtype=torch.float64)
    w = torch.zeros(3, 5, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride, pad, dil)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    torch.testing.assert_close(R.wgrad_einsum(x, dy.permute(0, 2, 3, 1).contiguous(), k, stride, pad, dil), w.grad, rtol=1e-12, atol=1e-12)


def test_float64_resnet_restatement_is_the_module_graph():
    """The stage restatement against the same stages written with nn modules in float64 (independent wiring: nn.Sequential order)."""
    import copy
    from sgv3d_amd.layers import blocks
    torch.manual_seed(0)
    r = blocks.ResNet(depth=18, base_channels=8, stem_channels=8, out_indices=(1, 3), frozen_stages=0, norm_eval=False)
    for m in r.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0, 0.3)
    x = torch.randn(2, 8, 12, 10, dtype=torch.float64)
    outs = R.resnet_stages(r, x)
    d = copy.deepcopy(r).double().train()
    want, h = [], x
    for i, name in enumerate(d.res_layers):
        for b in getattr(d, name):
            idn = h if b.downsample is None else b.downsample(h)
            o = F.relu(b.bn1(b.conv1(h)))
            h = F.relu(b.bn2(b.conv2(o)) + idn)
        if i in d.out_indices:
            want.append(h)
    assert len(outs) == len(want) == 2
    for a, b in zip(outs, want):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)
