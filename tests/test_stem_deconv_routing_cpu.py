"""CPU: the routing of SECONDFPN's transposed levels onto the f32x3 pointwise kernel (hip_ops.deconv_x3_eligible / deconv_x3 /
deconv_x3_choice): eligibility, signature strings, the fixed rule, the kill switch and what a launch hands the library -- on the
stand-in for the library the dispatch golden uses (tests/golden/make_golden_conv_dispatch.py)."""
import ctypes
import importlib.util
import os

import pytest
import torch

from conftest import GOLDEN


@pytest.fixture
def stage(monkeypatch):
    """hip_ops on the CPU stand-in, in the fp32 mode with every switch the eligibility reads at its default."""
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(GOLDEN, "make_golden_conv_dispatch.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with rec._cpu_stage() as (hip_ops, stand_in):
        for k, v in dict(MFMA_BF16=False, MFMA_F32X3=False, PW_X3=True, DECONV_X3=True, AUTOTUNE=True, SPLIT_K=True).items():
            monkeypatch.setattr(hip_ops, k, v)
        monkeypatch.setattr(hip_ops, "TUNE_DB", dict(hip_ops.TUNE_DB))
        monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: True)
        yield hip_ops, stand_in


def _level(hip_ops, cin=160, cout=64, ks=2, B=1, H=9, W=13, **kw):
    conv = hip_ops.PackedConv(torch.empty(cin, cout, ks, ks), stride=ks, transposed=True, relu=True, device="cpu", **kw)
    return conv, torch.empty(B, H, W, conv.cin)


def test_eligibility(stage, monkeypatch):
    hip_ops, _ = stage
    conv, x = _level(hip_ops)
    out = torch.empty(1, 18, 26, 256)
    assert hip_ops.deconv_x3_eligible(conv, x) and hip_ops.deconv_x3_eligible(conv, x, out, 64)
    assert hip_ops.deconv_x3_eligible(*_level(hip_ops, 32, 4, 8))
    for name, value in (("MFMA_BF16", True), ("PW_X3", False), ("DECONV_X3", False), ("MFMA_F32X3", True), ("MFMA_F32X3", "auto")):
        with monkeypatch.context() as m:
            m.setattr(hip_ops, name, value)
            assert not hip_ops.deconv_x3_eligible(conv, x), name
            assert hip_ops.deconv_x3_choice(conv, x) is None, name
    assert not hip_ops.deconv_x3_eligible(*_level(hip_ops, cin=176))                    # cin % 32 (SGV3D's padded 174-channel level)
    assert not hip_ops.deconv_x3_eligible(*_level(hip_ops, cout=38))                    # cout % 4
    plain = hip_ops.PackedConv(torch.empty(64, 160, 1, 1), device="cpu")                # not a transposed layer
    assert not hip_ops.deconv_x3_eligible(plain, x)
    assert not hip_ops.deconv_x3_eligible(conv, x.bfloat16())
    assert not hip_ops.deconv_x3_eligible(conv, x, out.bfloat16(), 64)
    assert not hip_ops.deconv_x3_eligible(conv, x, out, 62)                             # a misaligned channel offset
    assert not hip_ops.deconv_x3_eligible(conv, x, out, 224)                            # the window does not fit
    assert not hip_ops.deconv_x3_eligible(conv, x, torch.empty(1, 18, 27, 256), 0)      # not input * ks
    assert not hip_ops.deconv_x3_eligible(conv, x, torch.empty(1, 18, 26, 254), 0)


def test_signature_recorded_choices_and_the_fixed_rule(stage, monkeypatch):
    hip_ops, _ = stage
    for cin, cout, ks, B, H, W in ((2048, 128, 2, 1, 27, 48), (160, 64, 2, 1, 128, 128), (320, 64, 4, 8, 64, 64), (640, 64, 8, 1, 32, 32),
                                   (32, 4, 1, 2, 5, 7)):
        conv, x = _level(hip_ops, cin, cout, ks, B, H, W)
        sig = hip_ops.deconv_x3_signature(conv, x)
        assert sig == f"pair|deconv|{cout}x{cin}ks{ks}|{B}x{H}x{W}|r1|ts{hip_ops.TUNE_STREAMS}"
        gemm_m, gemm_n = B * H * W, ks * ks * cout
        rule = hip_ops._deconv_x3_rule(gemm_m, gemm_n)
        T = hip_ops.TILES[rule[0]]
        # 128 channels per workgroup, the largest m-tile that still gives every CU two workgroups, no split-K
        assert T.family == "pw_x3" and not T.mfirst and T.bn == 128 and rule[1] == 1
        wgs = lambda bm: -(-gemm_m // bm) * -(-gemm_n // 128)
        assert T.bm == next((bm for bm in (128, 64) if wgs(bm) >= 512), 32)
        with monkeypatch.context() as m:
            # a recorded choice is what the choice function returns: [0, 0] = the per-layer f32 choice, [1, 100 split-K + tile] = x3
            m.setitem(hip_ops.TUNE_DB, sig, [0, 0])
            assert hip_ops.deconv_x3_choice(conv, x) is None
            m.setitem(hip_ops.TUNE_DB, sig, [1, 161])
            assert hip_ops.deconv_x3_choice(conv, x) == (61, 1)
            if cin >= 96:
                m.setitem(hip_ops.TUNE_DB, sig, [1, 382])
                assert hip_ops.deconv_x3_choice(conv, x) == (82, 3)
            m.setitem(hip_ops.TUNE_DB, sig, [1, 171])                          # (m-tile first is not a form of this launch: the rule)
            assert hip_ops.deconv_x3_choice(conv, x) == rule
            m.setattr(hip_ops, "AUTOTUNE", False)                               # the fixed rule consults no record
            m.setitem(hip_ops.TUNE_DB, sig, [0, 0])
            assert hip_ops.deconv_x3_choice(conv, x) == rule
        # the candidates a measurement would time: plain tiles of the family only, split-K within the k-steps
        for t, splits in hip_ops._deconv_x3_candidates(gemm_m, gemm_n, cin // 32):
            assert t in hip_ops.PW_X3_TILES and not hip_ops.TILES[t].mfirst and splits[0] == 1
            assert all(s <= cin // 32 for s in splits)
    # deterministic mode: the rule, whatever the record says ... only where no record exists (a record is a measurement of this device)
    conv, x = _level(hip_ops, 96, 64, 2, 1, 40, 40)
    monkeypatch.setattr(hip_ops, "deterministic", lambda: True)
    assert hip_ops.deconv_x3_signature(conv, x) not in hip_ops.TUNE_DB
    assert hip_ops.deconv_x3_choice(conv, x) == hip_ops._deconv_x3_rule(1600, 256)
    assert hip_ops.deconv_x3_signature(conv, x) not in hip_ops.TUNE_DB       # nothing was measured, nothing written


def test_the_launch_hands_the_library_a_deconv_descriptor(stage):
    """``deconv_x3`` packs the [ks * ks * cout][cin] view once and calls sgv3d_conv2d_x3_forward with mode DECONV, the GEMM's
    cout_pad and the tile's ABI value; split-K brings a workspace of split * M * N floats."""
    from sgv3d_amd._lib import CONV_DECONV
    hip_ops, lib = stage
    conv, x = _level(hip_ops, 160, 64, 2, 2, 9, 13)
    out = torch.empty(2, 18, 26, 256)
    record = lib.sgv3d_conv2d_x3_forward
    descs = []

    def spy(d, *rest):                                       # (the stand-in writes down four fields of a descriptor: keep them all)
        descs.append({f: int(getattr(d._obj, f)) for f, _ in type(d._obj)._fields_})
        return record(d, *rest)
    lib.sgv3d_conv2d_x3_forward = spy
    hip_ops.deconv_x3(conv, x, out, 64)
    hip_ops.deconv_x3(conv, x, out, 64, tile=82, split_k=3)
    packs = [c for c in lib.calls if c[0] == "sgv3d_conv_pack_weight_x3"]
    assert len(packs) == 1 and packs[0][2:8] == [256, 160, 1, 1, 160, 256]               # rows = ks * ks * cout, packed once
    assert tuple(conv.w_pw_x3_deconv.shape) == (16, 5, 3, 512) and conv.w_pw_x3 is None
    runs = [c for c in lib.calls if c[0] == "sgv3d_conv2d_x3_forward"]
    assert len(runs) == 2
    rule = hip_ops._deconv_x3_rule(2 * 9 * 13, 256)
    for call, d, (tile, sk) in zip(runs, descs, (rule, (82, 3))):
        assert (d["mode"], d["deconv_ks"], d["cout"], d["cin"], d["cout_pad"]) == (CONV_DECONV, 2, 64, 160, 256)
        assert (d["in_h"], d["in_w"], d["out_h"], d["out_w"], d["y_ld"], d["y_coff"]) == (9, 13, 18, 26, 256, 64)
        assert (d["kh"], d["kw"], d["stride"], d["pad"], d["relu"], d["res_ld"]) == (1, 1, 1, 0, 1, 0)
        assert d["tile"] == hip_ops.TILES[tile].abi and d["split_k"] == sk
        assert call[6] == "-"                                                            # no residual
        assert (call[8], call[9]) == (("p", 4 * sk * 234 * 256) if sk > 1 else ("-", 0))
    with pytest.raises(Exception, match="not a tile of the f32x3 pointwise kernel"):
        hip_ops.deconv_x3(conv, x, out, 64, tile=4)


def test_secondfpn_routes_its_transposed_levels_and_the_kill_switch_stops_it(stage, monkeypatch):
    hip_ops, lib = stage
    from sgv3d_amd.layers.blocks import SECONDFPN
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)
    neck = SECONDFPN(in_channels=(32, 64, 96), out_channels=(32, 36, 64), upsample_strides=(1, 2, 4)).eval()
    feats = [torch.empty(1, 8 // s, 12 // s, c) for s, c in ((1, 32), (2, 64), (4, 96))]
    names = lambda: [c[0] for c in lib.calls if "forward" in c[0]]
    with torch.no_grad():
        neck.hip_forward(feats)
        assert names() == ["sgv3d_conv2d_forward", "sgv3d_conv2d_x3_forward", "sgv3d_conv2d_x3_forward"]
        del lib.calls[:]
        monkeypatch.setattr(hip_ops, "DECONV_X3", False)
        neck.hip_forward(feats)
        assert names() == ["sgv3d_conv2d_forward"] * 3


def test_refusals_of_the_entry_point_without_gpu():
    """The real library refuses what MODE 4 does not cover before any HIP call (the pointers are never dereferenced)."""
    from sgv3d_amd import _lib
    from sgv3d_amd._lib import ConvDesc, CONV_DECONV
    lib = _lib.load()

    def desc(**kw):
        d = ConvDesc()
        d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = 1, 5, 7, 32, 10, 14, 36
        d.kh, d.kw, d.stride, d.pad, d.dil = 1, 1, 1, 0, 1
        d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld, d.relu = 32, 0, 36, 0, 0, 1
        d.mode, d.deconv_ks, d.split_k, d.tile, d.k_pad, d.cout_pad, d.k_order = CONV_DECONV, 2, 1, 64 | 1, 32, 160, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, residual=None):
        rc = lib.sgv3d_conv2d_x3_forward(ctypes.byref(d), 0x1000, 0x1000, None, None, residual, 0x1000, None, 0, None)
        return rc, lib.sgv3d_last_error()
    for d, res, text in ((desc(), 0x1000, b"no residual"), (desc(cout=38, y_ld=40), None, b"cout % 4"),
                         (desc(cin=48, x_ld=48), None, b"cin % 32"), (desc(out_w=15), None, b"input * deconv_ks"),
                         (desc(out_h=5, out_w=7), None, b"input * deconv_ks"), (desc(deconv_ks=0), None, b"deconv_ks"),
                         (desc(stride=2), None, b"1x1 GEMM"), (desc(cout_pad=128), None, b"cout_pad"), (desc(split_k=2), None, b"split_k"),
                         (desc(y_ld=32), None, b"leading dimension too small")):
        rc, msg = call(d, res)
        assert rc == -1 and text in msg, (text, msg)


def test_every_key_the_new_code_writes_starts_with_pair(stage, monkeypatch):
    """A measurement (timed on the stand-in, where every launch takes no time) writes exactly one key, a ``pair|`` one holding two
    integers -- what the committed-DB tests and the dispatch golden's signature count rely on."""
    hip_ops, _ = stage
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: (fn(), 1.0)[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    conv, x = _level(hip_ops, 96, 64, 2, 1, 40, 40)
    conv.tile = 4                                           # (the per-layer side of the comparison: a fixed tile, nothing to measure)
    before = set(hip_ops.TUNE_DB)
    monkeypatch.setattr(hip_ops.PackedConv, "_autotune", lambda self, *a, **k: (4, 1))
    assert hip_ops.deconv_x3_choice(conv, x) is None        # a tie goes to the committed f32 choice
    new = {k: v for k, v in hip_ops.TUNE_DB.items() if k not in before and k.startswith("pair|")}
    assert list(new) == [hip_ops.deconv_x3_signature(conv, x)] and new[list(new)[0]] == [0, 0]
    assert all(k.startswith("pair|") or "|m1r0g0|" in k for k in set(hip_ops.TUNE_DB) - before)   # (+ the layer's own per-layer key)


def test_profile_record_of_the_x3_deconv(stage, monkeypatch):
    """Label ``conv_pw_x3_deconv`` with the layer's algorithmic flops and bytes, the MODE 4 symbol of the tile and the executed
    f32 / bf16 MFMA flops (six bf16 partial products per f32 product), as the other x3 labels carry them."""
    hip_ops, _ = stage
    conv, x = _level(hip_ops, 160, 64, 2, 2, 9, 13)
    out = torch.empty(2, 18, 26, 256)
    monkeypatch.setattr(hip_ops, "PROFILE", [])
    hip_ops.deconv_x3(conv, x, out, 64, tile=81, split_k=1)
    monkeypatch.setattr(hip_ops, "PROFILE_DETAIL", True)
    hip_ops.deconv_x3(conv, x, out, 64, tile=60, split_k=3)
    (name, flops, _, _, nbytes, extra), (detail, _, _, _, _, extra3) = hip_ops.PROFILE
    m, n, k = 2 * 9 * 13, 4 * 64, 160
    assert name == "conv_pw_x3_deconv" and name.startswith("conv_") and flops == 2.0 * m * n * k
    assert nbytes == 4.0 * (m * k + n * k + m * n)
    assert extra == {"symbol": "conv_pw_x3_kernel<4, 8, 4>", "mfma_flops": 2.0 * m * n * k, "bf16_mfma_flops": 12.0 * m * n * k}
    assert detail == "conv_pw_x3_deconv|2x9x13x160->64 k-2 s1 d1 splitk3" and extra3["symbol"] == "conv_pw_x3_kernel<2, 4, 4>"
