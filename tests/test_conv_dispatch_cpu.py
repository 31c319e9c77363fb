"""CPU: the convolution dispatch (sgv3d_amd.hip_ops.PackedConv over sgv3d_amd/conv_tiles.py) against its recorded behaviour.

tests/golden/make_golden_conv_dispatch.py runs every convolution signature of tune/gfx950_*.json, a sweep over all host tile ids,
layouts, modes and kill switches, and per kernel family a layer it does not cover, on ``device='cpu'`` against a stand-in for the
library; tests/golden/conv_dispatch.json.gz is what that gave before the tile ids had one table.  Equality, entry by entry: candidate
lists in order, the fixed rule's choice, the library calls with ``desc.tile`` / ``split_k`` / ``k_pad`` / ``cout_pad`` as passed, the
profile label / flops / bytes / symbol, the exceptions and their messages."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(GOLDEN, "make_golden_conv_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dispatch():
    rec = _recorder()
    with open(os.path.join(GOLDEN, "conv_dispatch.json.gz"), "rb") as f:
        want = rec.loads(f.read())
    got = json.loads(json.dumps(rec.record()))          # (tuples -> lists, as the file has them)
    return rec, got, want


def test_every_recorded_case_is_reproduced(dispatch):
    _, got, want = dispatch
    assert list(got) == list(want)
    assert len(want) >= 780 + 150
    for name in want:
        assert got[name] == want[name], name


def test_the_record_covers_every_committed_signature_and_every_tile_id(dispatch):
    """What the golden is worth: all convolution signatures of the committed tune DBs ran without error with a choice that is among
    their candidates, every host tile id was launched on a layer its family covers, every family refused one it does not."""
    from sgv3d_amd import conv_tiles, hip_ops
    rec, got, _ = dispatch
    committed, sweep = rec.committed_cases(), rec.sweep_cases()
    n_sigs = 0
    for f in os.listdir(os.path.join(ROOT, "tune")):
        if f.startswith("gfx950_") and f.endswith(".json"):
            with open(os.path.join(ROOT, "tune", f)) as fh:
                n_sigs += sum(1 for s in json.load(fh) if not s.startswith(("centerhead_branches", "wgrad|", "pair|")))
    assert len(committed) == n_sigs >= 780
    for name, case in committed.items():
        r = got[name]
        assert "error" not in r and r["calls"], name
        assert any(str(case["tile"]) in entry.split(":")[0].split() and str(case["split"]) in entry.split(":")[1].split(",")
                   for entry in r["cands"].split(";")), name
    launched = {case["tile"] for name, case in dict(committed, **sweep).items() if "error" not in got[name]}
    assert launched == set(conv_tiles.TILES) == set(hip_ops.TILE_NAMES)
    refused = {name.split(":")[0].split()[1] for name in sweep if name.startswith("refused ") and "error" in got[name]}
    assert refused == set(conv_tiles.FAMILIES)
    assert all("error" in got[name] for name in sweep if name.startswith("refused "))


def test_recording_leaves_the_process_as_it_was():
    import torch
    from sgv3d_amd import _lib, hip_ops
    before = (_lib.load, _lib.stream_handle, torch.cuda.device, torch.cuda.Event, hip_ops.MFMA_BF16, hip_ops.PROFILE, hip_ops.WINOGRAD)
    rec = _recorder()
    with rec._cpu_stage() as (ops, stand_in):
        assert _lib.load() is stand_in and ops is hip_ops
    assert before == (_lib.load, _lib.stream_handle, torch.cuda.device, torch.cuda.Event, hip_ops.MFMA_BF16, hip_ops.PROFILE, hip_ops.WINOGRAD)
