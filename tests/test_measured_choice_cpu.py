"""CPU: how a kernel that competes with another way of doing the same work is chosen -- SGV3D_NO_AUTOTUNE gives the fixed rule, else
the tune DB's entry (a committed one on gfx950 only), else the fixed rule in a capture / deterministic mode, else a measurement that
is written back -- at the sites no other routing test covers (conv_pair_choice, _wgrad_choice, BEVHeightHead._branch_path), the
functions every site is written on (hip_ops.tune_lookup / tune_may_measure / tune_record / tune_best_of) and the candidate list of
the f32x3 pointwise family against a frozen copy of its three former spellings.  On the stand-in for the library the dispatch golden
uses (tests/golden/make_golden_conv_dispatch.py)."""
import importlib.util
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN


@pytest.fixture
def stage(monkeypatch):
    """hip_ops on the CPU stand-in with a private TUNE_DB / committed set / counters, on a "gfx950 device", outside any capture."""
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(GOLDEN, "make_golden_conv_dispatch.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with rec._cpu_stage() as (hip_ops, stand_in):
        for k, v in dict(MFMA_BF16=False, MFMA_F32X3=False, PW_X3=True, AUTOTUNE=True, SPLIT_K=True, MFIRST=True, DETERMINISTIC=False).items():
            monkeypatch.setattr(hip_ops, k, v)
        monkeypatch.setattr(hip_ops, "TUNE_DB", {})
        monkeypatch.setattr(hip_ops, "_COMMITTED_SIGS", set())
        monkeypatch.setattr(hip_ops, "TUNE_STATS", {"measured": 0, "from_db": 0})
        monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: True)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        yield hip_ops, stand_in


def _no_clock(monkeypatch, hip_ops):
    monkeypatch.setattr(hip_ops, "time_callable", lambda *a, **k: pytest.fail("measured"))


# ------------------------------------------------------------------------------------------------ conv_pair_choice (bf16 mode)

def _pair(hip_ops, monkeypatch):
    """An eligible pair at its smallest: 3x3 32 -> 256 with ReLU, 1x1 256 -> 256, a 1x8x8x32 bf16 map; both layers with a fixed tile and
    their per-layer choice already made, so that the two-launch side of the comparison neither measures nor counts."""
    monkeypatch.setattr(hip_ops, "MFMA_BF16", True)
    monkeypatch.setattr(hip_ops.PackedConv, "_autotune", lambda self, *a, **k: (4, 1))
    a = hip_ops.PackedConv(torch.empty(256, 32, 3, 3), pad=1, relu=True, device="cpu", tile=4)
    b = hip_ops.PackedConv(torch.empty(256, 256, 1, 1), device="cpu", tile=4)
    x = torch.empty(1, 8, 8, 32, dtype=torch.bfloat16)
    b(a(x, out_dtype=torch.bfloat16), out_dtype=torch.bfloat16)
    sig = f"pair|256x32k3x3s1p1d1->256|1x8x8|r0|bf16|ts{hip_ops.TUNE_STREAMS}"
    return a, b, x, sig


def test_pair_recorded_choice_and_the_fixed_rule(stage, monkeypatch):
    hip_ops, _ = stage
    a, b, x, sig = _pair(hip_ops, monkeypatch)
    assert hip_ops.conv_pair_eligible(a, b, x)
    stats = dict(hip_ops.TUNE_STATS)
    _no_clock(monkeypatch, hip_ops)
    hip_ops.TUNE_DB[sig] = [0, 0]
    assert hip_ops.conv_pair_choice(a, b, x) is False
    hip_ops.TUNE_DB[sig] = [1, 0]
    assert hip_ops.conv_pair_choice(a, b, x) is True
    with monkeypatch.context() as m:                                            # the fixed rule consults no record
        m.setattr(hip_ops, "AUTOTUNE", False)
        hip_ops.TUNE_DB[sig] = [0, 0]
        assert hip_ops.conv_pair_choice(a, b, x) is True
    # a committed entry counts on a gfx950 device only: elsewhere the pair is as good as unrecorded (here: a capture's fixed rule)
    hip_ops._COMMITTED_SIGS.add(sig)
    assert hip_ops.conv_pair_choice(a, b, x) is False
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "_is_gfx950", lambda device: False)
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        assert hip_ops.conv_pair_choice(a, b, x) is True
    assert hip_ops.TUNE_DB[sig] == [0, 0] and sig in hip_ops._COMMITTED_SIGS
    # a capture / deterministic mode that meets a new signature: fused, nothing measured or written
    del hip_ops.TUNE_DB[sig]
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        assert hip_ops.conv_pair_choice(a, b, x) is True
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "deterministic", lambda: True)
        assert hip_ops.conv_pair_choice(a, b, x) is True
    assert sig not in hip_ops.TUNE_DB and hip_ops.TUNE_STATS == stats
    assert hip_ops.conv_pair_choice(a, b, x.float()) is False                  # not eligible: never fused


def test_pair_measurement(stage, monkeypatch):
    hip_ops, lib = stage
    a, b, x, sig = _pair(hip_ops, monkeypatch)
    stats = dict(hip_ops.TUNE_STATS)
    hip_ops._COMMITTED_SIGS.add(sig)
    clock = iter((2.0, 1.0))                                                    # two launches, then the fused one
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: next(clock))
    assert hip_ops.conv_pair_choice(a, b, x) is True
    assert hip_ops.TUNE_DB[sig] == [1, 0] and type(hip_ops.TUNE_DB[sig]) is list
    assert sig not in hip_ops._COMMITTED_SIGS                                   # measured on this device: no longer arch-bound
    del hip_ops.TUNE_DB[sig]
    lib.calls.clear()
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: (fn(), 1.0)[1])
    assert hip_ops.conv_pair_choice(a, b, x) is False                           # a tie goes to the two launches
    assert hip_ops.TUNE_DB[sig] == [0, 0]
    names = [c[0] for c in lib.calls if "pack" not in c[0]]
    two, one = [names[0], names[1]], ["sgv3d_conv_dw_bf16_pair_forward"]
    assert one[0] not in two and names == two + one + two + one                # both sides run once, then each is timed once
    assert hip_ops.TUNE_STATS == stats                                          # this site counts nothing


# ------------------------------------------------------------------------------------------------ conv_grad._wgrad_choice (lookup)

def _wgrad(hip_ops, monkeypatch):
    from sgv3d_amd import _lib, conv_grad
    monkeypatch.setattr(conv_grad, "_WGRAD_DB", {})
    d = _lib.ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = 1, 8, 8, 32, 8, 8, 64
    d.kh, d.kw, d.stride, d.pad, d.dil, d.x_ld, d.y_ld = 3, 3, 1, 1, 1, 32, 64
    x, dy = torch.empty(1, 8, 8, 32), torch.empty(1, 8, 8, 64)
    return conv_grad, d, x, dy, "wgrad|1x8x8x32x8x8x64x3x3x1x1x1x32x64"


def test_wgrad_lookup(stage, monkeypatch):
    hip_ops, lib = stage
    conv_grad, d, x, dy, sig = _wgrad(hip_ops, monkeypatch)
    with monkeypatch.context() as m:                                            # the library's own rule, whatever the DB holds
        m.setattr(hip_ops, "AUTOTUNE", False)
        hip_ops.TUNE_DB[sig] = [3, 2]
        assert conv_grad._wgrad_choice(lib, d, x, dy) == (0, 0) and conv_grad._WGRAD_DB == {}
    got = conv_grad._wgrad_choice(lib, d, x, dy)
    assert got == (3, 2) and type(got) is tuple and list(conv_grad._WGRAD_DB.values()) == [(3, 2)]
    hip_ops.TUNE_DB[sig] = [1, 4]
    assert conv_grad._wgrad_choice(lib, d, x, dy) == (3, 2)                     # (the per-shape copy answers from now on)
    # bf16 products / bf16 tensors: signatures of their own
    hip_ops.TUNE_DB[sig + "xbf16"] = [4, 1]
    assert conv_grad._wgrad_choice(lib, d, x, dy, bf16=True) == (4, 1)
    hip_ops.TUNE_DB[sig + "xbf16xt16"] = (6, 0)
    assert conv_grad._wgrad_choice(lib, d, x.bfloat16(), dy.bfloat16(), bf16=True) == (6, 0)


def test_wgrad_capture_and_a_committed_entry_elsewhere(stage, monkeypatch):
    hip_ops, lib = stage
    conv_grad, d, x, dy, sig = _wgrad(hip_ops, monkeypatch)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        assert conv_grad._wgrad_choice(lib, d, x, dy) == (0, 0)
        hip_ops.TUNE_DB[sig] = [3, 2]
        hip_ops._COMMITTED_SIGS.add(sig)
        m.setattr(hip_ops, "_is_gfx950", lambda device: False)
        assert conv_grad._wgrad_choice(lib, d, x, dy) == (0, 0)                 # committed, not gfx950: as good as unrecorded
    with monkeypatch.context() as m:
        m.setattr(hip_ops, "deterministic", lambda: True)
        m.setattr(hip_ops, "_is_gfx950", lambda device: False)
        assert conv_grad._wgrad_choice(lib, d, x, dy) == (0, 0)
    assert conv_grad._WGRAD_DB == {} and hip_ops.TUNE_DB == {sig: [3, 2]} and sig in hip_ops._COMMITTED_SIGS
    assert conv_grad._wgrad_choice(lib, d, x, dy) == (3, 2)                     # ... and on gfx950 it is used


# ------------------------------------------------------------------------------------------------ BEVHeightHead._branch_path

def _head(hip_ops, monkeypatch, f4=True, wino4=True):
    """The head's state as far as ``_branch_path`` reads it, and a log of which branch path ran."""
    from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead
    ran = []
    first = SimpleNamespace(cin=64, wino4_ok=lambda: wino4)
    s = dict(u_f4=torch.empty(1) if f4 else None, first=first, w2=None, b2=None, out_begin=None, nb=9)
    me = SimpleNamespace(_two_kernel_branches=lambda s, shared: ran.append(1), _fused_f4=lambda s, shared: ran.append(2))
    monkeypatch.setattr(hip_ops, "centerhead_branches", lambda *a, **k: ran.append(0))
    shared = torch.empty(1, 16, 24, 64)
    sig = f"centerhead_branches3|1x16x24x9|ts{hip_ops.TUNE_STREAMS}"
    return (lambda: BEVHeightHead._branch_path(me, s, shared)), sig, ran


def test_head_path_setting_record_and_rule(stage, monkeypatch):
    hip_ops, _ = stage
    _no_clock(monkeypatch, hip_ops)
    path, sig, ran = _head(hip_ops, monkeypatch)
    hip_ops.TUNE_DB[sig] = (101, 1)
    for want in (0, 1, 2):                                                      # an explicit setting wins over the record
        monkeypatch.setattr(hip_ops, "HEAD_PATH", want)
        assert path() == want
    monkeypatch.setattr(hip_ops, "HEAD_PATH", 2)
    assert _head(hip_ops, monkeypatch, f4=False)[0]() == 0                      # (... but F(4x4) only where it is available)
    monkeypatch.setattr(hip_ops, "HEAD_PATH", None)
    for k in (0, 1, 2):
        hip_ops.TUNE_DB[sig] = (100 + k, 1)
        assert path() == k
    with monkeypatch.context() as m:                                            # the fixed rule consults no record
        m.setattr(hip_ops, "AUTOTUNE", False)
        assert path() == 2 and _head(hip_ops, monkeypatch, f4=False)[0]() == 0
    # a recorded path that is not available here is not used: in a capture / deterministic mode the rule instead
    for patch in ((torch.cuda, "is_current_stream_capturing", lambda: True), (hip_ops, "deterministic", lambda: True)):
        with monkeypatch.context() as m:
            m.setattr(*patch)
            hip_ops.TUNE_DB[sig] = (102, 1)
            assert _head(hip_ops, monkeypatch, f4=False)[0]() == 0
            hip_ops.TUNE_DB[sig] = (101, 1)
            assert _head(hip_ops, monkeypatch, wino4=False)[0]() == 2
            del hip_ops.TUNE_DB[sig]
            assert path() == 2 and _head(hip_ops, monkeypatch, f4=False)[0]() == 0
    assert hip_ops.TUNE_DB == {} and ran == []


def test_head_path_measurement(stage, monkeypatch):
    hip_ops, _ = stage
    monkeypatch.setattr(hip_ops, "HEAD_PATH", None)
    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: synced.append(device))
    clock, seen = iter((3.0, 1.0, 2.0)), []
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: (seen.append(rounds), next(clock))[1])
    stats = dict(hip_ops.TUNE_STATS)
    path, sig, ran = _head(hip_ops, monkeypatch)
    assert path() == 1 and hip_ops.TUNE_DB[sig] == (101, 1) and type(hip_ops.TUNE_DB[sig]) is tuple
    assert ran == [0, 1, 2] and len(synced) == 1 and seen == [2, 2, 2]       # every path warmed once, in order, then timed
    assert path() == 1 and ran == [0, 1, 2]                                     # ... and recorded: not measured again
    # only the available paths compete; the first of equal times wins
    del hip_ops.TUNE_DB[sig]
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: 1.0)
    path, sig, ran = _head(hip_ops, monkeypatch, wino4=False)
    assert path() == 0 and ran == [0, 2] and hip_ops.TUNE_DB[sig] == (100, 1)
    assert hip_ops.TUNE_STATS == stats                                          # this site counts nothing


# ------------------------------------------------------------------------------------------------ the four shared functions

def test_lookup_and_record(stage, monkeypatch):
    hip_ops, _ = stage
    dev = torch.device("cpu")
    assert hip_ops.tune_lookup("a|sig", dev) is None                            # no entry
    hip_ops.TUNE_DB["a|sig"] = [1, 2]
    assert hip_ops.tune_lookup("a|sig", dev) is hip_ops.TUNE_DB["a|sig"]        # the entry as stored
    with monkeypatch.context() as m:                                            # SGV3D_NO_AUTOTUNE: no record is consulted
        m.setattr(hip_ops, "AUTOTUNE", False)
        m.setattr(hip_ops, "_is_gfx950", lambda device: pytest.fail("asked for the device"))
        assert hip_ops.tune_lookup("a|sig", dev) is None
    hip_ops._COMMITTED_SIGS.add("a|sig")
    asked = []
    monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: (asked.append(device), False)[1])
    assert hip_ops.tune_lookup("a|sig", dev) is None and asked == [dev]         # committed, and not a gfx950 device
    monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: True)
    assert hip_ops.tune_lookup("a|sig", dev) == [1, 2]
    # a record is a measurement on this device: it clears the committed mark
    hip_ops.tune_record("a|sig", (3, 4))
    assert hip_ops.TUNE_DB["a|sig"] == (3, 4) and "a|sig" not in hip_ops._COMMITTED_SIGS
    monkeypatch.setattr(hip_ops, "_is_gfx950", lambda device: pytest.fail("asked for the device"))
    assert hip_ops.tune_lookup("a|sig", dev) == (3, 4)
    # the functions read the module's TUNE_DB / _COMMITTED_SIGS when called: dicts swapped in are the ones they see
    other, marks = {"b|sig": [0, 0]}, {"c|sig"}
    monkeypatch.setattr(hip_ops, "TUNE_DB", other)
    monkeypatch.setattr(hip_ops, "_COMMITTED_SIGS", marks)
    assert hip_ops.tune_lookup("a|sig", dev) is None and hip_ops.tune_lookup("b|sig", dev) == [0, 0]
    hip_ops.tune_record("c|sig", [1, 1])
    assert other == {"b|sig": [0, 0], "c|sig": [1, 1]} and marks == set()


def test_may_measure(stage, monkeypatch):
    hip_ops, _ = stage
    assert hip_ops.tune_may_measure()
    for target, name, value in ((hip_ops, "AUTOTUNE", False), (hip_ops, "deterministic", lambda: True), (hip_ops, "DETERMINISTIC", True),
                                (torch.cuda, "is_current_stream_capturing", lambda: True)):
        with monkeypatch.context() as m:
            m.setattr(target, name, value)
            assert not hip_ops.tune_may_measure(), name
    assert hip_ops.tune_may_measure()


def test_best_of_order_and_ties(stage, monkeypatch, capsys):
    hip_ops, _ = stage
    log = []
    thunk = lambda name: (lambda: log.append(name))

    def clock(times):
        it = iter(times)

        def time_callable(fn, device, rounds=None):
            assert device == "dev" and rounds is None
            log.append("time")
            fn()
            return next(it)
        monkeypatch.setattr(hip_ops, "time_callable", time_callable)

    cands = [(k, thunk(k)) for k in ("a", "b", "c")]
    clock((5.0, 3.0, 2.0, 2.0))
    assert hip_ops.tune_best_of("s|ig", "dev", thunk("base"), cands) == (5.0, "b", 2.0)     # the first of equal candidates
    # the baseline is run once and timed, then every candidate in the given order: run once, then timed
    assert log == ["base", "time", "base", "a", "time", "a", "b", "time", "b", "c", "time", "c"]
    clock((2.0, 3.0, 2.0, 4.0))
    t0, best, t1 = hip_ops.tune_best_of("s|ig", "dev", thunk("base"), cands)
    assert (t0, best, t1) == (2.0, "b", 2.0) and not t1 < t0                                # a tie with the baseline: the caller keeps it
    clock((2.0, 3.0))
    assert hip_ops.tune_best_of("s|ig", "dev", thunk("base"), [((7, 2), thunk("x"))]) == (2.0, (7, 2), 3.0)
    assert capsys.readouterr().out == ""
    # SGV3D_TUNE_VERBOSE: one line per candidate with the signature, the candidate and both times in microseconds per launch
    monkeypatch.setattr(hip_ops, "TUNE_VERBOSE", True)
    monkeypatch.setattr(hip_ops, "TUNE_ROUNDS", 2)
    clock((0.5, 0.25))
    hip_ops.tune_best_of("s|ig", "dev", thunk("base"), [((7, 2), thunk("x"))])
    line = capsys.readouterr().out.strip()
    assert line.startswith("[tune] s|ig: ") and "(7, 2)" in line and "125.0 us" in line and "250.0 us" in line and "\n" not in line


def test_measured_sites_bind_their_loop_variable(stage, monkeypatch):
    """The candidate thunks are built before they are called: each must launch ITS tile (conv_shortcut_choice, two tiles to time)."""
    hip_ops, lib = stage
    monkeypatch.setattr(hip_ops.PackedConv, "_autotune", lambda self, *a, **k: (4, 1))
    c3 = hip_ops.PackedConv(torch.empty(256, 64, 1, 1), relu=True, device="cpu", scale=torch.empty(256), shift=torch.empty(256))
    ds = hip_ops.PackedConv(torch.empty(256, 64, 1, 1), device="cpu", scale=torch.empty(256), shift=torch.empty(256))
    mid, x = torch.empty(1, 96, 96, 64), torch.empty(1, 96, 96, 64)
    tiles = hip_ops._shortcut_tiles(96 * 96, 256)
    assert len(tiles) > 1
    seen = []
    real = hip_ops.conv_shortcut_x3
    monkeypatch.setattr(hip_ops, "conv_shortcut_x3", lambda *a, tile=None, **k: (seen.append(tile), real(*a, tile=tile, **k))[1])
    clock = iter([1.0] + [2.0] * (len(tiles) - 1) + [0.5])                       # the last tile is the fastest
    monkeypatch.setattr(hip_ops, "time_callable", lambda fn, device, rounds=None: (fn(), next(clock))[1])
    assert hip_ops.conv_shortcut_choice(c3, ds, mid, x) == tiles[-1]
    assert seen == [t for t in tiles for _ in (0, 1)]
    assert hip_ops.TUNE_DB[hip_ops.conv_shortcut_signature(c3, ds, x)] == [1, tiles[-1]]
    assert hip_ops.TUNE_STATS["measured"] >= 1                                   # this site counts (and so do the layers it warms)


# ------------------------------------------------------------------------------------------------ the pointwise family's candidates

def _frozen_candidates(hip_ops, gemm_m, gemm_n, nkt):
    """The three loops as they stood before they became one function (hip_ops.PackedConv._candidates' pw_x3 part with the split-K
    list of its common tail, _shortcut_tiles, _deconv_x3_candidates), copied unchanged but for the ``hip_ops.`` prefixes."""
    from sgv3d_amd import conv_tiles
    PW_X3_TILES, PW_X3_DIMS, TILES, SPLIT_K, MFIRST = hip_ops.PW_X3_TILES, hip_ops.PW_X3_DIMS, hip_ops.TILES, hip_ops.SPLIT_K, hip_ops.MFIRST
    # PackedConv._candidates
    tiles = ()
    for t in PW_X3_TILES:
        bm, bn = PW_X3_DIMS[t]
        wgs = -(-gemm_m // bm) * -(-gemm_n // bn)
        if bn == 256 and gemm_n < 256:
            continue
        if (wgs >= 96 or (SPLIT_K and nkt >= 16)) and (bn >= 128 or gemm_n <= 64 or wgs < 1024) and (not TILES[t].mfirst or (MFIRST and gemm_n > bn)):
            tiles += (t,)
    layer = []
    for t in tiles:
        T = TILES[t]
        wgs = -(-gemm_m // T.bm) * -(-gemm_n // T.bn)
        nk = nkt
        if not SPLIT_K:
            splits = (1,)
        else:
            pol = conv_tiles.SPLIT_POLICY[T.split]
            splits = [1] + [s for s in conv_tiles.SPLITS if nk // s >= pol["min_k"] and wgs < pol["max_wgs"] and wgs * s <= pol["max_total"]]
        layer.append((t, tuple(splits)))
    # _shortcut_tiles
    out = []
    for t in PW_X3_TILES:
        bm, bn = PW_X3_DIMS[t]
        wgs = -(-gemm_m // bm) * -(-gemm_n // bn)
        if (bm, bn) == (128, 64) or (bn == 256 and gemm_n < 256) or wgs < 96:
            continue
        if (bn >= 128 or gemm_n <= 64 or wgs < 1024) and (not TILES[t].mfirst or (MFIRST and gemm_n > bn)):
            out.append(t)
    shortcut = tuple(out) or (hip_ops._shortcut_rule_tile(gemm_m, gemm_n),)
    # _deconv_x3_candidates
    pol = conv_tiles.SPLIT_POLICY["igemm"]
    out = []
    for t in PW_X3_TILES:
        bm, bn = PW_X3_DIMS[t]
        wgs = -(-gemm_m // bm) * -(-gemm_n // bn)
        if TILES[t].mfirst or (bn == 256 and gemm_n < 256):
            continue
        if (wgs >= 96 or (SPLIT_K and nkt >= 16)) and (bn >= 128 or gemm_n <= 64 or wgs < 1024):
            splits = (1,) + (tuple(s for s in conv_tiles.SPLITS if nkt // s >= pol["min_k"] and wgs < pol["max_wgs"]
                                   and wgs * s <= pol["max_total"]) if SPLIT_K else ())
            out.append((t, splits))
    deconv = tuple(out) or ((hip_ops._shortcut_rule_tile(gemm_m, gemm_n), (1,)),)
    return layer, shortcut, deconv


@pytest.mark.parametrize("split_k, mfirst", list(itertools.product((True, False), repeat=2)))
def test_pointwise_candidates_are_the_three_former_lists(stage, monkeypatch, split_k, mfirst):
    hip_ops, _ = stage
    from sgv3d_amd import _lib
    monkeypatch.setattr(hip_ops, "SPLIT_K", split_k)
    monkeypatch.setattr(hip_ops, "MFIRST", mfirst)
    seen = set()
    for gemm_n in (4, 64, 128, 256, 512, 1024):
        conv = hip_ops.PackedConv(torch.empty(gemm_n, 64, 1, 1), device="cpu")         # a 1x1 layer the pointwise kernel covers
        d = _lib.ConvDesc()
        d.mode, d.x_ld, d.y_ld, d.cout, d.cin = hip_ops.CONV_NORMAL, 64, gemm_n, gemm_n, 64
        assert conv.pw_x3_ok(d)
        for gemm_m, nkt in itertools.product((1, 16, 31, 32, 1024, 12288, 24576, 65536, 221184), (1, 2, 15, 16, 64)):
            layer, shortcut, deconv = _frozen_candidates(hip_ops, gemm_m, gemm_n, nkt)
            got = [c for c in conv._candidates(d, None, gemm_m, gemm_n, nkt, 0, 0) if c[0] in hip_ops.PW_X3_TILES]
            assert got == layer, (gemm_m, gemm_n, nkt)
            assert hip_ops._shortcut_tiles(gemm_m, gemm_n) == shortcut, (gemm_m, gemm_n)
            assert hip_ops._deconv_x3_candidates(gemm_m, gemm_n, nkt) == deconv, (gemm_m, gemm_n, nkt)
            assert all(type(s) is tuple for _, s in got + list(hip_ops._deconv_x3_candidates(gemm_m, gemm_n, nkt)))
            seen.update(t for t, _ in layer)
            seen.update(shortcut)
    assert seen == set(hip_ops.PW_X3_TILES) or not mfirst                              # (the enumeration reaches every tile)
