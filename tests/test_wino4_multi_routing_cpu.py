"""CPU: the routing of sibling F(4x4) layers onto the multi entry point (hip_ops.wino4_multi_eligible / wino4_multi_choice, which
ASPP.hip_forward asks for its three dilated branches): what selects it, the switch, the recorded choice and the fixed rule, and the
entry point's host refusals -- on the stand-in for the library the dispatch golden uses (tests/golden/make_golden_conv_dispatch.py)."""
import ctypes
import importlib.util
import os

import pytest
import torch

from conftest import GOLDEN


@pytest.fixture
def stage(monkeypatch):
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(GOLDEN, "make_golden_conv_dispatch.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with rec._cpu_stage() as (hip_ops, stand_in):
        for k, v in dict(MFMA_BF16=False, MFMA_F32X3=False, WINO4=True, WINOGRAD=True, WINO4_X3=True, WINO4_MULTI=True, PARALLEL_BRANCHES=False,
                         AUTOTUNE=True).items():
            monkeypatch.setattr(hip_ops, k, v)
        monkeypatch.setattr(hip_ops, "TUNE_DB", dict(hip_ops.TUNE_DB))
        monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: True)
        yield hip_ops, stand_in


def _branch(hip_ops, dil, cout=512, cin=512, k=3, **kw):
    return hip_ops.PackedConv(torch.empty(cout, cin, k, k), pad=dil if k == 3 else 0, dil=dil, relu=True, device="cpu",
                              scale=torch.empty(cout), shift=torch.empty(cout), **kw)


def _group(hip_ops, dils=(6, 12, 18)):
    return [_branch(hip_ops, d) for d in dils]


def _record(hip_ops, convs, x, picks):
    B, H, W, _ = x.shape
    for c, p in zip(convs, picks):
        c._tile_cache[(B, H, W, 0, 0, False, False, hip_ops.CONV_NORMAL, False, False, 0)] = p


X = torch.empty(1, 54, 96, 512)
CAT = torch.empty(1, 54, 96, 2048)
OFFS = [512, 1024, 1536]


def test_eligibility_and_every_refusal(stage, monkeypatch):
    hip_ops, _ = stage
    convs = _group(hip_ops)
    assert hip_ops.wino4_multi_eligible(convs, X, CAT, OFFS) and hip_ops.wino4_multi_eligible(convs[:2], X)
    for name, value in (("MFMA_BF16", True), ("MFMA_F32X3", True), ("MFMA_F32X3", "auto"), ("WINO4_X3", False), ("WINO4_MULTI", False),
                        ("WINO4", False), ("WINOGRAD", False), ("PARALLEL_BRANCHES", True)):
        with monkeypatch.context() as m:
            m.setattr(hip_ops, name, value)
            assert not hip_ops.wino4_multi_eligible(convs, X, CAT, OFFS), name
            assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) is None, name
    assert not hip_ops.wino4_multi_eligible(convs, X, CAT, OFFS, training=True)
    assert not hip_ops.wino4_multi_eligible(convs[:1], X, CAT, OFFS[:1])                       # one layer: nothing to share
    assert not hip_ops.wino4_multi_eligible(_group(hip_ops, (1, 2, 3, 6, 12)), X)              # five
    assert not hip_ops.wino4_multi_eligible(convs[:2] + [_branch(hip_ops, 18, cin=256)], X)    # another input width
    assert not hip_ops.wino4_multi_eligible(convs[:2] + [_branch(hip_ops, 1, k=1)], X)         # a 1x1 layer
    assert not hip_ops.wino4_multi_eligible(convs[:2] + [_branch(hip_ops, 1, cout=64, cin=64)], torch.empty(1, 54, 96, 64))
    assert not hip_ops.wino4_multi_eligible(convs, X.bfloat16(), CAT, OFFS) and not hip_ops.wino4_multi_eligible(convs, X[0], CAT, OFFS)
    assert not hip_ops.wino4_multi_eligible(convs, X, CAT.bfloat16(), OFFS)
    assert not hip_ops.wino4_multi_eligible(convs, X, torch.empty(1, 54, 95, 2048), OFFS)      # another map
    assert not hip_ops.wino4_multi_eligible(convs, X, CAT, [512, 1024, 1538])                  # offset % 4
    assert not hip_ops.wino4_multi_eligible(convs, X, CAT, [512, 1024, 1540])                  # past the buffer
    assert not hip_ops.wino4_multi_eligible(convs, X, CAT, OFFS[:2]) and not hip_ops.wino4_multi_eligible(convs, X, CAT, None)
    with monkeypatch.context() as m:
        before = hip_ops.switch_state()
        m.setattr(hip_ops, "WINO4_MULTI", False)
        assert hip_ops.switch_state() != before                                                # part of a recorded graph's key


def test_the_layers_choices_select_it(stage, monkeypatch):
    hip_ops, _ = stage
    convs = _group(hip_ops)
    x3 = list(hip_ops.WINO4_X3_TILES)
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)                                            # the fixed rule: no record, no timing
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) is None                             # choices not known yet: per layer
    _record(hip_ops, convs, X, [(x3[1], 1), (x3[0], 1), (x3[7], 1)])
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) == (x3[1], x3[0], x3[7])
    assert hip_ops.wino4_multi_choice(convs, torch.empty(2, 54, 96, 512), torch.empty(2, 54, 96, 2048), OFFS) is None   # another batch
    for bad in ((hip_ops.TILE_WINO4, 1), (4, 1), (x3[0], 2), (0, 0)):                          # f32 F(4x4), implicit GEMM, split-K, unknown
        _record(hip_ops, convs, X, [(x3[1], 1), bad, (x3[7], 1)])
        assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) is None, bad
    fixed = [_branch(hip_ops, d, tile=x3[2]) for d in (6, 12, 18)]                             # tiles given to the layers themselves
    assert hip_ops.wino4_multi_choice(fixed, X, CAT, OFFS) == (x3[2],) * 3


def test_recorded_choice_fixed_rule_and_signature(stage, monkeypatch):
    hip_ops, _ = stage
    convs = _group(hip_ops)
    x3 = list(hip_ops.WINO4_X3_TILES)
    _record(hip_ops, convs, X, [(x3[1], 1)] * 3)
    sig = hip_ops.wino4_multi_signature(convs, X)
    assert sig == f"pair|wino4multi|512x512d6+512x512d12+512x512d18|1x54x96|ts{hip_ops.TUNE_STREAMS}"
    monkeypatch.setattr(hip_ops, "tune_may_measure", lambda: False)                            # a capture / deterministic mode
    hip_ops.TUNE_DB.pop(sig, None)
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) == (x3[1],) * 3                     # fixed rule: the multi launch
    hip_ops.TUNE_DB[sig] = [0, 0]
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) is None                             # the record says per layer
    hip_ops.TUNE_DB[sig] = [1, 0]
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) == (x3[1],) * 3
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)                                            # SGV3D_NO_AUTOTUNE consults no record
    hip_ops.TUNE_DB[sig] = [0, 0]
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) == (x3[1],) * 3
    monkeypatch.setattr(hip_ops, "WINO4_MULTI", False)
    assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) is None


def test_measured_once_and_recorded(stage, monkeypatch):
    hip_ops, _ = stage
    convs = _group(hip_ops)
    x3 = list(hip_ops.WINO4_X3_TILES)
    _record(hip_ops, convs, X, [(x3[1], 1)] * 3)
    sig = hip_ops.wino4_multi_signature(convs, X)
    hip_ops.TUNE_DB.pop(sig, None)
    monkeypatch.setattr(hip_ops, "tune_may_measure", lambda: True)
    for times, want, entry in (((10.0, 9.0), (x3[1],) * 3, [1, 0]), ((9.0, 9.0), None, [0, 0])):   # only strictly faster wins
        hip_ops.TUNE_DB.pop(sig, None)
        calls = []
        monkeypatch.setattr(hip_ops, "tune_best_of", lambda s, dev, base, cands: (calls.append((s, [k for k, _ in cands])), (times[0], 1, times[1]))[1])
        assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) == want
        assert hip_ops.TUNE_DB[sig] == entry and calls == [(sig, [1])]
        assert hip_ops.wino4_multi_choice(convs, X, CAT, OFFS) == want and len(calls) == 1        # from the record now


def test_committed_entries_are_well_formed():
    import glob
    import json
    from conftest import ROOT
    for f in glob.glob(os.path.join(ROOT, "tune", "gfx950_*.json")):
        for sig, val in json.load(open(f)).items():
            if sig.startswith("pair|wino4multi|"):
                assert len(val) == 2 and val[0] in (0, 1) and val[1] == 0, (sig, val)


def test_refusals_of_the_entry_point_without_gpu():
    """The real library refuses before any HIP call (the pointers are never dereferenced)."""
    from sgv3d_amd import _lib
    from sgv3d_amd._lib import ConvDesc
    lib = _lib.load()

    def descs(n, **over):
        a = (ConvDesc * max(n, 1))()
        for l in range(max(n, 1)):
            d = a[l]
            d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = 1, 7, 19, 128, 7, 19, 128
            d.kh, d.kw, d.stride, d.pad, d.dil = 3, 3, 1, (1, 6, 12, 18)[l % 4], (1, 6, 12, 18)[l % 4]
            d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld, d.relu, d.mode = 128, 0, 512, 128 * (l % 4), 0, 1, 0
            d.k_pad, d.cout_pad, d.tile, d.k_order, d.split_k = 128, 128, 0, 1, 1
        return a

    from sgv3d_amd import hip_ops
    X3 = hip_ops.TILES[hip_ops.WINO4_X3_TILES[1]].abi

    def call(n, a, ws=1 << 30, x=0x1000, ptrs=0x1000, edit=None, null_arrays=False):
        for l in range(max(n, 1)):
            a[l].tile = X3
        if edit:
            edit(a)
        arr = (ctypes.c_void_p * 4)(*([ptrs] * 4))
        pa = None if null_arrays else ctypes.addressof(arr)
        return lib.sgv3d_conv2d_winograd4_forward_multi(n, ctypes.addressof(a), x, pa, pa, pa, pa, 0x1000, ws, None)

    need = lib.sgv3d_conv2d_winograd4_multi_workspace_bytes
    a = descs(3)
    for l in range(3):
        a[l].tile = X3
    assert need(3, ctypes.addressof(a)) > 0 and need(0, ctypes.addressof(a)) == 0 and need(5, ctypes.addressof(a)) == 0
    single = [lib.sgv3d_conv2d_winograd4_workspace_bytes(ctypes.byref(a[l])) for l in range(3)]
    assert need(3, ctypes.addressof(a)) == sum((b + 255) // 256 * 256 for b in single)
    cases = [
        (dict(n=0, a=descs(1)), -1, b"1 to 4 layers"), (dict(n=5, a=descs(5)), -1, b"1 to 4 layers"),
        (dict(n=3, a=descs(3), x=None), -1, b"null pointer"), (dict(n=3, a=descs(3), null_arrays=True), -1, b"null pointer"),
        (dict(n=3, a=descs(3), ptrs=None), -1, b"null pointer"), (dict(n=3, a=descs(3), ptrs=0x1004), -1, b"aligned"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[2], "in_w", 20) or setattr(a[2], "out_w", 20)), -1, b"same input"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[1], "x_coff", 4) or setattr(a[1], "x_ld", 132)), -1, b"same input"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[1], "batch", 2)), -1, b"same input"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[1], "tile", 4)), -1, b"SGV3D_TILE_X3"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[0], "mode", 3)), -1, b"NHWC output"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[0], "pad", 2)), -1, b"pad == dilation"),
        (dict(n=3, a=descs(3), edit=lambda a: setattr(a[2], "y_coff", 448)), -1, b"leading dimension too small"),
        (dict(n=3, a=descs(3), ws=need(3, ctypes.addressof(a)) - 1), -3, b"workspace has"),
    ]
    for kw, code, text in cases:
        rc = call(**kw)
        assert rc == code and text in lib.sgv3d_last_error(), (kw, rc, lib.sgv3d_last_error())
