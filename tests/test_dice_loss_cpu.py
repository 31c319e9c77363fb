"""CPU side of losses.DiceLoss (csrc/dice_loss.hip): the float64 restatement the GPU tests compare against
(tests/dice_ref.py) is pinned to the reference's own values and autograd gradients (tests/golden/dice_loss.npz, written by
tests/golden/make_golden_dice.py); the C ABI's declarations, its host-side rejections and the Python layer's contract are
checked without a GPU."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dice_ref
from conftest import GOLDEN, ROOT

GOLD = np.load(os.path.join(GOLDEN, "dice_loss.npz"))
CASES = sorted(k[:-5] for k in GOLD.files if k.endswith("_loss"))


def _kw(name):
    return ast.literal_eval(str(GOLD[name + "_kw"]))


# ----------------------------------------------------------------------------------------------- fixture and restatement
def test_fixture_holds_the_cases_and_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "dice_loss.npz")) < 300 * 1024
    kws = {n: _kw(n) for n in CASES}
    assert kws["bsm"] == dict(mode='multiclass') and GOLD["bsm_x"].shape[1] == 7
    k = kws["mc_log_smooth_ignore"]
    assert k["log_loss"] and k["smooth"] == 1.0 and k["ignore_index"] == 255
    share = float((GOLD["mc_log_smooth_ignore_y"] == 255).mean())
    assert 0.1 < share < 0.3
    assert kws["mc_classes"]["classes"] == [1, 2, 6]
    rep = kws["mc_classes_repeat"]["classes"]
    assert len(set(rep)) < len(rep)
    assert 2 not in GOLD["mc_absent_class_y"] and GOLD["mc_absent_class_x"].shape[1] > 2
    assert (GOLD["mc_all_ignored_y"] == kws["mc_all_ignored"]["ignore_index"]).all()
    assert float(GOLD["mc_all_ignored_loss"]) == 0 and not GOLD["mc_all_ignored_grad"].any()
    assert kws["bin_smooth"]["mode"] == "binary" and 0 < kws["bin_smooth"]["smooth"] < 0.1
    assert kws["ml_ignore"]["ignore_index"] == 255 and (GOLD["ml_ignore_y"] == 255).any()
    y = GOLD["ml_soft_log_y"]
    assert y.dtype == np.float32 and ((y > 0) & (y < 1)).any()
    assert {kws[n]["mode"] for n in CASES if kws[n].get("from_logits") is False} == {"multiclass", "multilabel"}
    assert set(np.unique(GOLD["mc_pm300_x"])) == {-300.0, 300.0}
    for n in CASES:
        assert GOLD[n + "_x"].dtype == np.float32 and GOLD[n + "_grad"].dtype == np.float64
        assert GOLD[n + "_grad32"].dtype == np.float32 and np.isfinite(GOLD[n + "_grad"]).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name):
    x = torch.from_numpy(GOLD[name + "_x"]).double().requires_grad_(True)
    y = torch.from_numpy(GOLD[name + "_y"])
    loss = dice_ref.dice_loss(x, y, **_kw(name))
    loss.backward()
    assert abs(float(loss.detach()) - float(GOLD[name + "_loss"])) <= 1e-12
    assert float((x.grad - torch.from_numpy(GOLD[name + "_grad"])).abs().max()) <= 1e-12


def test_restatement_takes_uint8_labels_and_out_of_range_ids():
    x = torch.from_numpy(GOLD["mc_log_smooth_ignore_x"]).double()
    y = torch.from_numpy(GOLD["mc_log_smooth_ignore_y"])
    kw = _kw("mc_log_smooth_ignore")
    assert float(dice_ref.dice_loss(x, y.to(torch.uint8), **kw)) == float(dice_ref.dice_loss(x, y, **kw))
    # an id outside [0, C) that is not the ignore index matches no class: its pixel still counts in P
    free = dice_ref.dice_loss(x, y, **dict(kw, ignore_index=None))
    assert abs(float(free) - float(GOLD["mc_log_smooth_ignore_loss"])) > 1e-3


# ----------------------------------------------------------------------------------------------- C ABI
_CTYPE = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
          "float": ctypes.c_float}


def _header_protos():
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|size_t)\s+(sgv3d_dice_loss_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            if "*" in a:
                types.append(ctypes.c_void_p)
            else:
                types.append(_CTYPE[a.rsplit(" ", 1)[0].replace("const ", "")])
        out[name] = (_CTYPE[res], types)
    return out


def test_header_and_ctypes_agree():
    from sgv3d_amd import _lib
    protos = _header_protos()
    assert sorted(protos) == ["sgv3d_dice_loss_backward", "sgv3d_dice_loss_forward", "sgv3d_dice_loss_workspace_bytes"]
    for name, (res, args) in protos.items():
        got_res, got_args = _lib._PROTOS[name]
        assert got_res is res, name
        assert len(got_args) == len(args), (name, len(got_args), len(args))
        assert list(got_args) == args, name
    assert len(protos["sgv3d_dice_loss_forward"][1]) == 21 and len(protos["sgv3d_dice_loss_backward"][1]) == 18


P = 64      # a stand-in for a device pointer: every refusal below comes before anything is dereferenced or launched


def _forward(lib, batch=1, classes=7, pixels=8, pred=P, target=P, kind=0, act=2, weight=P, out=P, saved=P, ws=P, nws=None):
    nws = lib.sgv3d_dice_loss_workspace_bytes(classes) if nws is None else nws
    return lib.sgv3d_dice_loss_forward(batch, classes, pixels, pred, classes * pixels, pixels, 1, target, kind, act, 0, 0, 0.0,
                                       1e-7, 0, weight, out, saved, ws, nws, None)


def _backward(lib, batch=1, classes=7, pixels=8, pred=P, target=P, kind=0, act=2, saved=P, grad=P):
    return lib.sgv3d_dice_loss_backward(batch, classes, pixels, pred, classes * pixels, pixels, 1, target, kind, act, 0, 0, 0.0,
                                        1e-7, saved, None, grad, None)


REFUSALS = [
    (dict(batch=0), b"bad sizes"), (dict(classes=0), b"bad sizes"), (dict(pixels=-3), b"bad sizes"),
    (dict(pred=None), b"null pointer"), (dict(target=None), b"null pointer"),
    (dict(kind=3), b"target_kind"), (dict(kind=-1), b"target_kind"), (dict(act=3), b"activation"),
    (dict(classes=33), b"2..32 classes"), (dict(classes=1), b"2..32 classes"),
    (dict(kind=2), b"softmax needs integer labels"),
    (dict(kind=0, act=1), b"integer labels need softmax"), (dict(kind=1, act=0), b"integer labels need softmax"),
]


@pytest.mark.parametrize("change,message", REFUSALS)
def test_bad_arguments_are_refused_by_name_without_a_gpu(change, message):
    from sgv3d_amd import _lib
    lib = _lib.load()
    for call, who in ((_forward, b"dice_loss_forward"), (_backward, b"dice_loss_backward")):
        assert call(lib, **change) == -1
        err = lib.sgv3d_last_error()
        assert message in err and who in err, err


def test_null_outputs_and_short_workspace_are_refused_without_a_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    for name in ("weight", "out", "saved", "ws"):
        assert _forward(lib, **{name: None}) == -1 and b"null pointer" in lib.sgv3d_last_error()
    for name in ("saved", "grad"):
        assert _backward(lib, **{name: None}) == -1 and b"null pointer" in lib.sgv3d_last_error()
    need = lib.sgv3d_dice_loss_workspace_bytes(7)
    assert need >= 7 * 3 * 8 and need % 8 == 0
    assert lib.sgv3d_dice_loss_workspace_bytes(14) == 2 * need and lib.sgv3d_dice_loss_workspace_bytes(0) == 0
    assert _forward(lib, nws=need - 1) == -3 and b"workspace too small" in lib.sgv3d_last_error()
    with pytest.raises(_lib.SGV3DError, match="workspace too small"):
        _lib.check(_forward(lib, nws=0), "sgv3d_dice_loss_forward")


# ----------------------------------------------------------------------------------------------- Python layer
def test_dice_covers_rule():
    from sgv3d_amd import hip_ops
    assert [c for c in range(0, 40) if hip_ops.dice_covers("multiclass", c)] == list(range(2, 33))
    for mode in ("binary", "multilabel"):
        assert hip_ops.dice_covers(mode, 1) and hip_ops.dice_covers(mode, 33) and hip_ops.dice_covers(mode, 1000)
        assert not hip_ops.dice_covers(mode, 0)
    assert not hip_ops.dice_covers("jaccard", 7)


def test_the_import_line_of_the_reference_resolves():
    from sgv3d_amd.losses import DiceLoss            # noqa: F401  (fails without the feature)
    import sgv3d_amd.losses as L
    assert "DiceLoss" in L.__all__ and L.DiceLoss.__module__ == "sgv3d_amd.losses.dice"


def test_cpu_tensors_raise():
    from sgv3d_amd.losses import DiceLoss
    with pytest.raises(RuntimeError, match="MI355X only"):
        DiceLoss('multiclass')(torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long))
    with pytest.raises(RuntimeError, match="MI355X only"):
        DiceLoss('binary')(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))


def test_constructor_keeps_the_reference_conditions_and_defaults():
    import inspect
    from sgv3d_amd.losses import DiceLoss
    with pytest.raises(AssertionError):
        DiceLoss('jaccard')
    with pytest.raises(AssertionError, match="not supported with mode=binary"):
        DiceLoss('binary', classes=[0])
    sig = inspect.signature(DiceLoss.__init__)
    assert list(sig.parameters)[1:] == ["mode", "classes", "log_loss", "from_logits", "smooth", "ignore_index", "eps"]
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == dict(
        classes=None, log_loss=False, from_logits=True, smooth=0.0, ignore_index=None, eps=1e-7)
    d = DiceLoss('multilabel', classes=torch.tensor([2, 0, 2]))
    assert d.classes == [2, 0, 2]
    # the class weights: multiplicity / length, float32; an index past the channels raises as indexing the losses would
    w = d._class_weight(3, torch.device("cpu"))
    assert w.dtype == torch.float32 and w.tolist() == [np.float32(1 / 3), 0.0, np.float32(2 / 3)]
    with pytest.raises(IndexError):
        d._class_weight(2, torch.device("cpu"))
    assert DiceLoss('multiclass')._class_weight(7, torch.device("cpu")).tolist() == [float(np.float32(1 / 7))] * 7


def test_semantic_supervision_default_has_no_dice_object():
    from sgv3d_amd.losses import DiceLoss, SemanticSupervision
    s = SemanticSupervision(8)
    assert s.dice_loss is None and s.dice_weight == 0.0
    assert not any(isinstance(m, DiceLoss) for m in s.modules())
    s = SemanticSupervision(8, dice_weight=0.5, dice_kwargs=dict(smooth=1.0, ignore_index=255))
    assert isinstance(s.dice_loss, DiceLoss) and s.dice_loss.mode == 'multiclass'
    assert s.dice_loss.smooth == 1.0 and s.dice_loss.ignore_index == 255
