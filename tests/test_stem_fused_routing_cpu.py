"""CPU: the routing of the image stem onto the one-launch kernel (hip_ops.stem_fused_eligible / stem_fused / stem_fused_choice,
ResNet.hip_forward_image): eligibility, the signature string, the recorded choice and the fixed rule, the kill switch and what a
launch hands the library -- on the stand-in for the library the dispatch golden uses (tests/golden/make_golden_conv_dispatch.py)."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT


@pytest.fixture
def stage(monkeypatch):
    """hip_ops on the CPU stand-in, in the fp32 mode with every switch the eligibility reads at its default."""
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(GOLDEN, "make_golden_conv_dispatch.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with rec._cpu_stage() as (hip_ops, stand_in):
        for k, v in dict(MFMA_BF16=False, MFMA_F32X3=False, PW_X3=True, STEM_FUSED=True, AUTOTUNE=True, SPLIT_K=True).items():
            monkeypatch.setattr(hip_ops, k, v)
        monkeypatch.setattr(hip_ops, "TUNE_DB", dict(hip_ops.TUNE_DB))
        monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: True)
        yield hip_ops, stand_in


def _stem(hip_ops, cout=64, cin=3, k=7, stride=2, pad=3, dil=1, relu=True, affine=True, **kw):
    return hip_ops.PackedConv(torch.empty(cout, cin, k, k), stride=stride, pad=pad, dil=dil, relu=relu, device="cpu",
                              scale=torch.empty(cout) if affine else None, shift=torch.empty(cout) if affine else None, **kw)


def test_eligibility_and_every_refusal(stage, monkeypatch):
    hip_ops, _ = stage
    conv, x = _stem(hip_ops), torch.empty(2, 3, 37, 53)
    assert hip_ops.stem_fused_eligible(conv, x) and hip_ops.stem_fused_eligible(conv, torch.empty(1, 3, 1, 1))
    for name, value in (("MFMA_BF16", True), ("PW_X3", False), ("STEM_FUSED", False), ("MFMA_F32X3", True), ("MFMA_F32X3", "auto")):
        with monkeypatch.context() as m:
            m.setattr(hip_ops, name, value)
            assert not hip_ops.stem_fused_eligible(conv, x), name
            assert hip_ops.stem_fused_choice(conv, x) is None, name
    assert not hip_ops.stem_fused_eligible(conv, x, act_dtype=torch.bfloat16)           # a network that keeps bf16 activations
    assert not hip_ops.stem_fused_eligible(conv, x, maxpool=False)                      # the BEV trunk: no max-pool behind the stem
    for other in (dict(k=3, pad=1), dict(stride=1), dict(pad=2), dict(dil=2, pad=6), dict(cout=32), dict(cout=128), dict(cin=4),
                  dict(cin=80, cin_pad=80), dict(relu=False), dict(affine=False), dict(cin_pad=8)):
        assert not hip_ops.stem_fused_eligible(_stem(hip_ops, **other), x), other
    only_shift = hip_ops.PackedConv(torch.empty(64, 3, 7, 7), stride=2, pad=3, relu=True, device="cpu", shift=torch.empty(64))
    assert not hip_ops.stem_fused_eligible(only_shift, x)                               # a bias, no folded BN
    deconv = hip_ops.PackedConv(torch.empty(32, 64, 2, 2), stride=2, transposed=True, relu=True, device="cpu")
    assert not hip_ops.stem_fused_eligible(deconv, x)
    assert not hip_ops.stem_fused_eligible(conv, x.double()) and not hip_ops.stem_fused_eligible(conv, x.bfloat16())
    assert not hip_ops.stem_fused_eligible(conv, torch.empty(2, 4, 37, 53))             # 4 planes
    assert not hip_ops.stem_fused_eligible(conv, torch.empty(2, 37, 53, 3).permute(0, 3, 1, 2))   # NHWC memory behind an NCHW view
    assert not hip_ops.stem_fused_eligible(conv, torch.empty(3, 37, 53))
    assert not hip_ops.stem_fused_eligible(conv, torch.empty(0, 3, 37, 53))
    with monkeypatch.context() as m:
        before = hip_ops.switch_state()
        m.setattr(hip_ops, "STEM_FUSED", False)
        assert hip_ops.switch_state() != before                                         # part of a recorded graph's key


def test_signature_recorded_choice_and_the_fixed_rule(stage, monkeypatch):
    hip_ops, _ = stage
    conv = _stem(hip_ops)
    for B, H, W in ((1, 864, 1536), (8, 864, 1536), (2, 37, 53)):
        x = torch.empty(B, 3, H, W)
        sig = hip_ops.stem_fused_signature(conv, x)
        assert sig == f"pair|stem|64x3k7|{B}x{H}x{W}|ts{hip_ops.TUNE_STREAMS}"
        with monkeypatch.context() as m:
            m.setitem(hip_ops.TUNE_DB, sig, [0, 0])
            assert hip_ops.stem_fused_choice(conv, x) is None
            m.setitem(hip_ops.TUNE_DB, sig, [1, 0])
            assert hip_ops.stem_fused_choice(conv, x) == 0
            m.setitem(hip_ops.TUNE_DB, sig, [1, 7])                            # (not a variant of this build: the rule's)
            assert hip_ops.stem_fused_choice(conv, x) == 0
            m.setattr(hip_ops, "AUTOTUNE", False)                               # the fixed rule consults no record
            m.setitem(hip_ops.TUNE_DB, sig, [0, 0])
            assert hip_ops.stem_fused_choice(conv, x) == 0
    # deterministic mode / a capture that meets a new signature: the rule, and nothing is measured or written
    x = torch.empty(1, 3, 41, 43)
    sig = hip_ops.stem_fused_signature(conv, x)
    assert sig not in hip_ops.TUNE_DB
    monkeypatch.setattr(hip_ops, "time_callable", lambda *a, **k: pytest.fail("measured"))
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "deterministic", lambda: True)
        assert hip_ops.stem_fused_choice(conv, x) == 0
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        assert hip_ops.stem_fused_choice(conv, x) == 0
    assert sig not in hip_ops.TUNE_DB


def test_a_measurement_writes_one_pair_key_of_two_slots(stage, monkeypatch):
    """Timed on the stand-in, where every launch takes no time: a tie goes to the three launches."""
    hip_ops, lib = stage
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: (fn(), 1.0)[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    conv, x = _stem(hip_ops), torch.empty(1, 3, 41, 43)
    conv.tile = 4                                           # (the per-layer side of the comparison: a fixed tile, nothing to measure)
    monkeypatch.setattr(hip_ops.PackedConv, "_autotune", lambda self, *a, **k: (4, 1))
    before = set(hip_ops.TUNE_DB)
    assert hip_ops.stem_fused_choice(conv, x) is None
    new = {k: v for k, v in hip_ops.TUNE_DB.items() if k not in before and k.startswith("pair|")}
    assert list(new) == [hip_ops.stem_fused_signature(conv, x)] and new[list(new)[0]] == [0, 0]
    assert all(k.startswith("pair|") or "|m0r0g0|" in k for k in set(hip_ops.TUNE_DB) - before)   # (+ the layer's own per-layer key)
    names = [c[0] for c in lib.calls if "pack" not in c[0]]
    three = ["sgv3d_nchw_to_nhwc", "sgv3d_conv2d_forward", "sgv3d_maxpool3x3s2"]
    assert names == three * 2 + ["sgv3d_stem_pool_x3_forward"] * 2      # each side run once, then timed once
    # ... and a faster fused launch is recorded as [1, variant]
    clock = iter((2.0, 1.0))
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: next(clock))
    x2 = torch.empty(1, 3, 45, 43)
    assert hip_ops.stem_fused_choice(conv, x2) == 0 and hip_ops.TUNE_DB[hip_ops.stem_fused_signature(conv, x2)] == [1, 0]


def test_the_launch_hands_the_library_the_image_and_the_x3_pack(stage, monkeypatch):
    hip_ops, lib = stage
    conv, x = _stem(hip_ops), torch.empty(2, 3, 37, 53)
    out = hip_ops.stem_fused(conv, x)
    assert tuple(out.shape) == (2, 10, 14, 64) and out.dtype == torch.float32
    wide = torch.empty(2, 10, 14, 80)
    assert hip_ops.stem_fused(conv, x, out=wide, variant=0) is wide
    packs = [c for c in lib.calls if c[0] == "sgv3d_conv_pack_weight_x3"]
    assert len(packs) == 1 and packs[0][2:8] == [64, 3, 7, 7, 4, 64]                     # the tap-major pack, made once
    assert tuple(conv.w_pw_x3.shape) == (4, 7, 3, 512)
    runs = [c for c in lib.calls if c[0] == "sgv3d_stem_pool_x3_forward"]
    assert [r[1:] for r in runs] == [[2, 37, 53, "p", "p", 86016, "p", "p", "p", ld, 0, "p"] for ld in (64, 80)]
    with pytest.raises(Exception, match="unknown variant"):
        hip_ops.stem_fused(conv, x, variant=3)
    for h, w, want in ((1, 1, (1, 1)), (7, 9, (2, 3)), (8, 8, (2, 2)), (9, 10, (3, 3)), (864, 1536, (216, 384))):
        assert hip_ops.stem_fused_out_hw(h, w) == want
    # the profile record: label, algorithmic flops and bytes, the kernel's symbol and the flops it executes
    monkeypatch.setattr(hip_ops, "PROFILE", [])
    hip_ops.stem_fused(conv, x)
    monkeypatch.setattr(hip_ops, "PROFILE_DETAIL", True)
    hip_ops.stem_fused(conv, x)
    (name, flops, _, _, nbytes, extra), (detail, _, _, _, _, _) = hip_ops.PROFILE
    assert name == "conv_stem_fused" and flops == 2.0 * 2 * 19 * 27 * 64 * 147
    assert nbytes == 4.0 * (2 * 3 * 37 * 53 + 64 * 147 + 2 * 10 * 14 * 64)
    mfma = 2.0 * 2 * 3 * 1 * 20 * 16 * 64 * 224                   # 3 x 1 tiles per image, 20 groups of 16 conv pixels each
    assert extra == {"symbol": "stem_pool_x3_kernel<4, 16>", "mfma_flops": mfma, "bf16_mfma_flops": 6 * mfma}
    assert detail == "conv_stem_fused|2x37x53x3->64 k7 s2 + maxpool v0"


def test_resnet_takes_the_fused_launch_and_the_kill_switch_restores_the_three(stage, monkeypatch):
    hip_ops, lib = stage
    from sgv3d_amd.layers.blocks import ResNet
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)
    net = ResNet(depth=18).eval()
    x = torch.empty(1, 3, 37, 53)
    names = lambda: [c[0] for c in lib.calls if "pack" not in c[0]]
    with torch.no_grad():
        net.hip_forward(hip_ops.nchw_to_nhwc(x, c_pad=4), split_tag="t")
        before = names()
        assert before[:3] == ["sgv3d_nchw_to_nhwc", "sgv3d_conv2d_forward", "sgv3d_maxpool3x3s2"]
        del lib.calls[:]
        outs = net.hip_forward_image(x, split_tag="t")
        assert names() == ["sgv3d_stem_pool_x3_forward"] + before[3:] and len(outs) == 4
        del lib.calls[:]
        monkeypatch.setattr(hip_ops, "STEM_FUSED", False)
        net.hip_forward_image(x, split_tag="t")
        assert names() == before                                  # exactly today's call sequence
        del lib.calls[:]
        # a recorded [0, 0] keeps the three launches with the switch on
        monkeypatch.setattr(hip_ops, "STEM_FUSED", True)
        monkeypatch.setattr(hip_ops, "AUTOTUNE", True)
        monkeypatch.setattr(hip_ops, "deterministic", lambda: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        stem =net.hip_state(x.device)["stem"]
        monkeypatch.setitem(hip_ops.TUNE_DB, hip_ops.stem_fused_signature(stem, x), [0, 0])
        net.hip_forward_image(x, split_tag="t")
        assert names()[:3] == before[:3]
    # the BEV trunk's 80-channel stem is not this stem
    trunk = ResNet(depth=18, in_channels=80, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(0, 1, 2)).eval()
    assert not hip_ops.stem_fused_eligible(trunk.hip_state(x.device)["stem"], torch.empty(1, 80, 16, 16))


def test_every_committed_stem_entry_decodes_to_a_known_variant(stage):
    hip_ops, _ = stage
    seen = 0
    for name in sorted(os.listdir(os.path.join(ROOT, "tune"))):
        if not name.endswith(".json"):
            continue
        with open(os.path.join(ROOT, "tune", name)) as f:
            db = json.load(f)
        for sig, val in db.items():
            if not sig.startswith("pair|stem|"):
                continue
            seen += 1
            assert len(val) == 2 and val[0] in (0, 1) and (val[1] in hip_ops.STEM_FUSED_VARIANTS if val[0] else val[1] == 0), (sig, val)
            assert sig.split("|")[2] == "64x3k7"
    assert seen >= 2                                              # cfg-2 at batch 1 and 8


def test_refusals_of_the_entry_point_without_gpu():
    """The real library refuses before any HIP call (the pointers are never dereferenced)."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    good = dict(batch=1, h=9, w=10, x=0x1000, u=0x1000, nb=86016, sc=0x1000, sh=0x1000, y=0x1000, y_ld=64, variant=0)
    for kw, text in ((dict(x=None), b"null pointer"), (dict(u=None), b"null pointer"), (dict(y=None), b"null pointer"),
                     (dict(y_ld=60), b"y_ld"), (dict(y_ld=66), b"y_ld"), (dict(batch=0), b"bad shape"), (dict(h=0), b"bad shape"),
                     (dict(w=-3), b"bad shape"), (dict(variant=1), b"unknown variant"), (dict(nb=4096), b"weight pack"),
                     (dict(sc=None), b"scale and shift"), (dict(y=0x1004), b"aligned")):
        a = dict(good, **kw)
        rc = lib.sgv3d_stem_pool_x3_forward(a["batch"], a["h"], a["w"], a["x"], a["u"], a["nb"], a["sc"], a["sh"], a["y"], a["y_ld"],
                                            a["variant"], None)
        assert rc == -1 and text in lib.sgv3d_last_error(), (kw, lib.sgv3d_last_error())
