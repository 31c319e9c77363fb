"""CPU: the two-source launch of the f32x3 implicit-GEMM kernel (sgv3d_conv2d_x3_shortcut_forward, hip_ops.conv_shortcut_x3) refuses
bad arguments before any HIP call, its eligibility function says no where the launch does not apply, and its tune-DB signatures
are ``pair|`` ones."""
import ctypes

import pytest
import torch


def _desc(cin, cout, in_hw, out_hw, stride=1, batch=1, tile=64 | 1):
    from sgv3d_amd._lib import ConvDesc, CONV_NORMAL
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = batch, in_hw[0], in_hw[1], cin, out_hw[0], out_hw[1], cout
    d.kh, d.kw, d.stride, d.pad, d.dil = 1, 1, stride, 0, 1
    d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld, d.relu = cin, 0, cout, 0, 0, 1
    d.mode, d.split_k, d.tile, d.k_pad, d.cout_pad, d.k_order = CONV_NORMAL, 1, tile, cin, (cout + 31) // 32 * 32, 1
    return d


def _call(lib, da, db, ptrs=None):
    p = [0x1000] * 9 if ptrs is None else ptrs           # (never dereferenced: every case is refused on the host)
    xa, ua, sa, ha, xb, ub, sb, hb, y = p
    return lib.sgv3d_conv2d_x3_shortcut_forward(ctypes.byref(da), xa, ua, sa, ha, ctypes.byref(db), xb, ub, sb, hb, y, None)


def test_shortcut_entry_refuses_bad_arguments_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    good_a, good_b = _desc(64, 256, (5, 7), (5, 7)), _desc(128, 256, (9, 13), (5, 7), stride=2)
    for i in (0, 1, 4, 5, 8):                                                             # xa, u3a, xb, u3b, y
        ptrs = [0x1000] * 9
        ptrs[i] = None
        assert _call(lib, good_a, good_b, ptrs) == -1 and b"null pointer" in lib.sgv3d_last_error()
    assert lib.sgv3d_conv2d_x3_shortcut_forward(None, *[0x1000] * 4, ctypes.byref(good_b), *[0x1000] * 5, None) == -1
    assert b"null pointer" in lib.sgv3d_last_error()
    # the sources' output geometries differ: size, batch; a source whose output does not follow from its input and stride
    assert _call(lib, good_a, _desc(128, 256, (9, 16), (5, 8), stride=2)) == -1 and b"output geometries differ" in lib.sgv3d_last_error()
    assert _call(lib, good_a, _desc(128, 256, (9, 13), (5, 7), stride=2, batch=2)) == -1 and b"output geometries differ" in lib.sgv3d_last_error()
    assert _call(lib, good_a, _desc(128, 256, (9, 13), (9, 13), stride=2)) == -1 and b"does not match the geometry" in lib.sgv3d_last_error()
    # cout mismatch
    assert _call(lib, good_a, _desc(128, 512, (9, 13), (5, 7), stride=2)) == -1 and b"cout differ" in lib.sgv3d_last_error()
    # what the kernel does not cover: cin % 32, stride 3, a 3x3 source, split-K, a misaligned pointer, an unknown tile variant
    assert _call(lib, _desc(48, 256, (5, 7), (5, 7)), good_b) == -1 and b"cin % 32" in lib.sgv3d_last_error()
    assert _call(lib, good_a, _desc(128, 256, (13, 19), (5, 7), stride=3)) == -1 and b"stride 1 or 2" in lib.sgv3d_last_error()
    bad = _desc(128, 256, (9, 13), (5, 7), stride=2)
    bad.kh = bad.kw = 3
    assert _call(lib, good_a, bad) == -1 and b"1x1" in lib.sgv3d_last_error()
    bad = _desc(64, 256, (5, 7), (5, 7))
    bad.split_k = 2
    assert _call(lib, bad, good_b) == -1 and b"no split-K" in lib.sgv3d_last_error()
    assert _call(lib, good_a, good_b, [0x1000] * 8 + [0x1004]) == -1 and b"16-B aligned" in lib.sgv3d_last_error()
    assert _call(lib, _desc(64, 256, (5, 7), (5, 7), tile=64 | 3), good_b) == -1 and b"variant" in lib.sgv3d_last_error()
    assert _call(lib, _desc(64, 256, (5, 7), (5, 7), tile=1), good_b) == -1 and b"variant" in lib.sgv3d_last_error()


@pytest.fixture
def switches(monkeypatch):
    """hip_ops in the fp32 mode with every switch the eligibility reads at its default, whatever the environment says."""
    from sgv3d_amd import hip_ops
    for k, v in dict(MFMA_BF16=False, MFMA_F32X3=False, PW_X3=True, SHORTCUT_X3=True, AUTOTUNE=True).items():
        monkeypatch.setattr(hip_ops, k, v)
    return hip_ops


def _pair(hip_ops, cin_a=64, cin_b=256, cout=256, stride=2, **kw):
    c3 = hip_ops.PackedConv(torch.empty(cout, cin_a, 1, 1), relu=True, device="cpu")
    ds = hip_ops.PackedConv(torch.empty(cout, cin_b, 1, 1), stride=stride, device="cpu", **kw)
    x = torch.empty(2, 9, 13, cin_b)
    oh, ow = ds.out_hw(9, 13)
    return c3, ds, torch.empty(2, oh, ow, cin_a), x


def test_eligibility_says_no_where_the_launch_does_not_apply(switches, monkeypatch):
    hip_ops = switches
    c3, ds, mid, x = _pair(hip_ops)
    assert hip_ops.conv_shortcut_eligible(c3, ds, mid, x)
    assert hip_ops.conv_shortcut_eligible(*_pair(hip_ops, 32, 32, 36, 1))
    for name, value in (("MFMA_BF16", True), ("PW_X3", False), ("SHORTCUT_X3", False), ("MFMA_F32X3", True), ("MFMA_F32X3", "auto")):
        with monkeypatch.context() as m:
            m.setattr(hip_ops, name, value)
            assert not hip_ops.conv_shortcut_eligible(c3, ds, mid, x), name
            assert hip_ops.conv_shortcut_choice(c3, ds, mid, x) == 0, name
    assert not hip_ops.conv_shortcut_eligible(*_pair(hip_ops, cin_a=48))                 # cin % 32 != 0, either source
    assert not hip_ops.conv_shortcut_eligible(*_pair(hip_ops, cin_b=80))
    # a transposed layer (kernel == stride deconvolution), either side
    t = hip_ops.PackedConv(torch.empty(64, 256, 1, 1), stride=1, transposed=True, device="cpu")
    assert not hip_ops.conv_shortcut_eligible(t, ds, mid, x) and not hip_ops.conv_shortcut_eligible(c3, t, mid, x)
    # bf16 tensors, a shortcut with a ReLU, a 3x3 shortcut, another output size, another cout
    assert not hip_ops.conv_shortcut_eligible(c3, ds, mid.bfloat16(), x) and not hip_ops.conv_shortcut_eligible(c3, ds, mid, x.bfloat16())
    assert not hip_ops.conv_shortcut_eligible(*_pair(hip_ops, relu=True))
    k3 = hip_ops.PackedConv(torch.empty(256, 256, 3, 3), stride=2, pad=1, device="cpu")
    assert not hip_ops.conv_shortcut_eligible(c3, k3, mid, x)
    assert not hip_ops.conv_shortcut_eligible(c3, ds, torch.empty(2, 9, 13, 64), x)
    assert not hip_ops.conv_shortcut_eligible(hip_ops.PackedConv(torch.empty(128, 64, 1, 1), device="cpu"), ds, mid, x)


def test_signatures_are_pair_signatures_and_the_fixed_rule_is_fused(switches, monkeypatch):
    hip_ops = switches
    for args in ((64, 256, 256, 2), (64, 64, 256, 1), (32, 32, 36, 1), (512, 1024, 2048, 2)):
        c3, ds, mid, x = _pair(hip_ops, *args)
        sig = hip_ops.conv_shortcut_signature(c3, ds, x)
        assert sig.startswith("pair|shortcut|") and sig.endswith(f"|ts{hip_ops.TUNE_STREAMS}"), sig
        # a recorded choice is what the choice function returns: [0, 0] = two launches, [1, tile] = fused with that tile
        with monkeypatch.context() as m:
            m.setitem(hip_ops.TUNE_DB, sig, [0, 0])
            assert hip_ops.conv_shortcut_choice(c3, ds, mid, x) == 0
            m.setitem(hip_ops.TUNE_DB, sig, [1, 71])
            assert hip_ops.conv_shortcut_choice(c3, ds, mid, x) == 71
            m.setattr(hip_ops, "AUTOTUNE", False)                     # the fixed rule consults no record: fused, the rule's tile
            t = hip_ops.conv_shortcut_choice(c3, ds, mid, x)
            assert t in hip_ops.PW_X3_TILES and not hip_ops.TILES[t].mfirst and hip_ops.TILES[t].bn == 128
    # the rule's m-tile: the largest that still gives every CU two workgroups
    assert [hip_ops.TILES[hip_ops._shortcut_rule_tile(m, 256)].bm for m in (82944, 20736, 5184, 70)] == [128, 64, 32, 32]
    # every committed pair signature names a decision
    import glob
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in glob.glob(os.path.join(root, "tune", "gfx950_*.json")):
        for sig, (on, t) in json.load(open(f)).items():
            if sig.startswith("pair|shortcut|"):
                assert (on, t) == (0, 0) or (on == 1 and t in hip_ops.PW_X3_TILES and hip_ops.PW_X3_DIMS[t] != (128, 64)), (f, sig)
