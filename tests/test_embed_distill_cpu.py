"""CPU side of the embedding distillation (csrc/embed_distill.hip, sgv3d_amd/distill.py, losses.EmbedDistillation): the torch
restatement the GPU tests compare against (tests/embed_distill_ref.py) and the library's host twin are pinned to the reference's
own warp and loss (tests/golden/embed_distill.npz, written by tests/golden/make_golden_embed_distill.py); the C ABI's
declarations, its host-side rejections and the Python layer's contract are checked without a GPU."""
import ast
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import embed_distill_ref as ER
from conftest import GOLDEN, ROOT

GOLD = np.load(os.path.join(GOLDEN, "embed_distill.npz"))
CASES = sorted(k[:-6] for k in GOLD.files if k.endswith("_embed"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------- fixture and restatement
def test_fixture_holds_the_cases_and_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "embed_distill.npz")) < 1000000
    assert {tuple(GOLD[n + "_embed"].shape) for n in CASES} == {(5, 7, 4), (9, 13, 8), (17, 23, 36)}
    strong = [n for n in CASES if n.endswith("strong")]
    assert len(strong) == 3 and all(GOLD[n + "_args"][0] == 1.3 and GOLD[n + "_args"][1] == 4.0 for n in strong)
    shrink = [n for n in CASES if n.endswith("shrink")]
    assert shrink and all(GOLD[n + "_args"][0] < 1 and float(GOLD[n + "_dead_share"]) > 0.30 for n in shrink)
    ident = [n for n in CASES if n.endswith("identity")]
    assert ident and all(np.array_equal(GOLD[n + "_M"], np.eye(3)) for n in ident)
    for n in ident:             # the reference's identity warp zeroes the last row and column: why unwarped frames are copied
        out, src = GOLD[n + "_out"], GOLD[n + "_embed"]
        assert not out[-1].any() and not out[:, -1].any() and np.array_equal(out[:-1, :-1], src[:-1, :-1])
    for n in CASES:
        assert GOLD[n + "_out"].dtype == np.float32 and GOLD[n + "_grad"].dtype == np.float64
        assert GOLD[n + "_grad32"].dtype == np.float32 and GOLD[n + "_minv"].dtype == np.float64


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name):
    out, dead = ER.warp(torch.from_numpy(GOLD[name + "_embed"]), GOLD[name + "_minv"])
    assert np.array_equal(_bits(out.numpy()), _bits(GOLD[name + "_out"]))
    assert abs(float(dead.double().mean()) - float(GOLD[name + "_dead_share"])) < 1e-12
    s = torch.from_numpy(GOLD[name + "_student"]).double()[None].requires_grad_(True)
    loss = ER.distill_loss(s, out[None], dead[None], 1000.0)
    loss.backward()
    assert abs(float(loss.detach()) - float(GOLD[name + "_loss"])) <= 1e-12 * float(GOLD[name + "_loss"])
    assert float((s.grad[0] - torch.from_numpy(GOLD[name + "_grad"])).abs().max()) <= 1e-12


def test_restatement_mask_dead_drops_the_dead_pixels():
    name = "m_shrink"
    out, dead = ER.warp(torch.from_numpy(GOLD[name + "_embed"]), GOLD[name + "_minv"])
    s = torch.from_numpy(GOLD[name + "_student"]).double()[None].requires_grad_(True)
    loss = ER.distill_loss(s, out[None], dead[None], 1000.0, mask_dead=True)
    loss.backward()
    live = ~dead
    d = s.detach()[0][:, live] - out.double().permute(2, 0, 1)[:, live]
    assert abs(float(loss.detach()) - 1000.0 * float((d * d).mean())) < 1e-9
    assert not s.grad[0][:, dead].any() and s.grad[0][:, live].abs().min() > 0
    everything = torch.ones_like(dead)
    assert float(ER.distill_loss(s.detach(), out[None], everything[None], 1000.0, mask_dead=True)) == 0.0


@pytest.mark.parametrize("name", [n for n in CASES if not n.endswith("identity")])
def test_embed_warp_matrix_matches_the_reference(name):
    from sgv3d_amd.distill import embed_warp_matrix
    K, E, Kr, Er = (GOLD[name + k] for k in ("_K", "_E", "_Kr", "_Er"))
    got = embed_warp_matrix(K, E, Kr, Er, 1.0 / 16)                 # the reference's own function is the case 1/16
    assert got.dtype == np.float64 and got.shape == (3, 3)
    assert np.allclose(got, GOLD[name + "_minv"], rtol=1e-12, atol=1e-15)
    assert np.allclose(np.linalg.inv(got), GOLD[name + "_M"], rtol=1e-11, atol=1e-14)
    assert np.array_equal(got, ER.warp_matrix(K, E, Kr, Er, 1.0 / 16))
    # another grid scale is another matrix: the translation column scales, the linear part does not
    other = np.linalg.inv(embed_warp_matrix(K, E, Kr, Er, 0.05))
    assert np.allclose(other[:2, 2], GOLD[name + "_M"][:2, 2] * (0.05 * 16), rtol=1e-9, atol=1e-12)
    assert np.allclose(other[:2, :2], GOLD[name + "_M"][:2, :2], rtol=1e-9, atol=1e-12)


def test_embed_warp_matrices_follow_the_draws():
    from sgv3d_amd import synthetic, train_augment
    from sgv3d_amd.distill import embed_warp_matrices, embed_warp_matrix
    params = train_augment.AugmentParams([True, False, True], [1.2, 0, 0.9], [2.0, 0, -1.0], [0.5, 0, -0.2], [False] * 3, [0.0] * 3)
    cams = [synthetic.make_calib(pitch_deg=11.0 + b) for b in range(3)]
    rect = [train_augment.augment_camera(c, params, i) for i, c in enumerate(cams)]
    minv, warped = embed_warp_matrices(cams, rect, params, 0.05)
    assert minv.shape == (3, 3, 3) and minv.dtype == np.float64 and warped.dtype == np.uint8 and warped.tolist() == [1, 0, 1]
    assert np.array_equal(minv[1], np.eye(3))
    for i in (0, 2):
        want = embed_warp_matrix(cams[i]['intrin'], np.linalg.inv(np.asarray(cams[i]['sensor2ego'], np.float64)), rect[i]['intrin'],
                                 np.linalg.inv(np.asarray(rect[i]['sensor2ego'], np.float64)), 0.05)
        assert np.array_equal(minv[i], want) and not np.allclose(minv[i], np.eye(3), atol=1e-3)
    with pytest.raises(ValueError, match="cameras"):
        embed_warp_matrices(cams[:2], rect, params, 0.05)


# ----------------------------------------------------------------------------------------------- host twin
def _host_warp(lib, teacher, minv, warped, want_dead=True):
    teacher = np.ascontiguousarray(teacher, np.float32)
    b, h, w, c = teacher.shape
    minv = np.ascontiguousarray(minv, np.float64).reshape(b, 9)
    warped = np.ascontiguousarray(warped, np.uint8)
    out = np.full(teacher.shape, np.nan, np.float32)
    dead = np.full((b, h, w), 7, np.uint8)
    rc = lib.sgv3d_embed_warp_host(b, h, w, c, teacher.ctypes.data, minv.ctypes.data, warped.ctypes.data, out.ctypes.data,
                                   dead.ctypes.data if want_dead else None)
    assert rc == 0, lib.sgv3d_last_error()
    return out, dead


@pytest.mark.parametrize("name", CASES)
def test_host_twin_matches_the_reference(name):
    from sgv3d_amd import _lib
    lib = _lib.load()
    out, dead = _host_warp(lib, GOLD[name + "_embed"][None], GOLD[name + "_minv"][None], [1])
    assert np.array_equal(_bits(out[0]), _bits(GOLD[name + "_out"]))
    _, want_dead = ER.warp(torch.from_numpy(GOLD[name + "_embed"]), GOLD[name + "_minv"])
    assert np.array_equal(dead[0], want_dead.numpy().astype(np.uint8))


def test_host_twin_copies_unwarped_frames_and_takes_no_dead_map():
    from sgv3d_amd import _lib
    lib = _lib.load()
    e = GOLD["m_strong_embed"]
    teacher = np.stack([e, e[::-1].copy(), GOLD["m_shrink_embed"]])
    minv = np.stack([GOLD["m_strong_minv"], GOLD["m_shrink_minv"], GOLD["m_shrink_minv"]])
    out, dead = _host_warp(lib, teacher, minv, [1, 0, 1])
    assert np.array_equal(_bits(out[0]), _bits(GOLD["m_strong_out"]))
    assert np.array_equal(_bits(out[1]), _bits(teacher[1])) and not dead[1].any()          # the strong matrix is not applied
    assert np.array_equal(_bits(out[2]), _bits(GOLD["m_shrink_out"])) and dead[2].mean() > 0.3
    out2, untouched = _host_warp(lib, teacher, minv, [1, 0, 1], want_dead=False)
    assert np.array_equal(_bits(out2), _bits(out)) and (untouched == 7).all()
    # a matrix that is not a number kills its frame instead of indexing with it
    bad = minv.copy()
    bad[0, 2, 2] = np.nan
    out3, dead3 = _host_warp(lib, teacher, bad, [1, 0, 1])
    assert dead3[0].all() and not out3[0].any()


# ----------------------------------------------------------------------------------------------- C ABI
_CTYPE = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
          "float": ctypes.c_float}
NAMES = ["sgv3d_embed_distill_backward", "sgv3d_embed_distill_forward", "sgv3d_embed_distill_workspace_bytes", "sgv3d_embed_warp",
         "sgv3d_embed_warp_host"]


def _header_protos():
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|size_t)\s+(sgv3d_embed_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        types_ = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a == "void":
                continue
            types_.append(ctypes.c_void_p if "*" in a else _CTYPE[a.rsplit(" ", 1)[0].replace("const ", "")])
        out[name] = (_CTYPE[res], types_)
    return out


def test_header_and_ctypes_agree():
    from sgv3d_amd import _lib
    protos = _header_protos()
    assert sorted(protos) == NAMES
    for name, (res, args) in protos.items():
        got_res, got_args = _lib._PROTOS[name]
        assert got_res is res, name
        assert list(got_args) == args, name
    assert [len(protos[n][1]) for n in NAMES] == [16, 18, 0, 10, 9]
    lib = _lib.load()
    for n in NAMES:
        getattr(lib, n)


P = 64      # a stand-in for a device pointer (16-byte aligned): every refusal comes before anything is dereferenced or launched
FAR = 1 << 40


def _warp(lib, host, batch=1, h=4, w=6, c=8, teacher=P, minv=P, warped=P, out=FAR):
    if host:
        return lib.sgv3d_embed_warp_host(batch, h, w, c, teacher, minv, warped, out, None)
    return lib.sgv3d_embed_warp(batch, h, w, c, teacher, minv, warped, out, None, None)


def _forward(lib, batch=1, c=8, h=4, w=6, student=P, sb=None, sc=None, sp=1, teacher=FAR, minv=P, warped=P, weight=1000.0,
             out=P, saved=P, ws=P, nws=None):
    nws = lib.sgv3d_embed_distill_workspace_bytes() if nws is None else nws
    sc = h * w if sc is None else sc
    sb = c * h * w if sb is None else sb
    return lib.sgv3d_embed_distill_forward(batch, c, h, w, student, sb, sc, sp, teacher, minv, warped, weight, 0, out, saved, ws, nws,
                                           None)


def _backward(lib, batch=1, c=8, h=4, w=6, student=P, sb=None, sc=None, sp=1, teacher=FAR, minv=P, warped=P, saved=P, grad=P):
    sc = h * w if sc is None else sc
    sb = c * h * w if sb is None else sb
    return lib.sgv3d_embed_distill_backward(batch, c, h, w, student, sb, sc, sp, teacher, minv, warped, 0, saved, None, grad, None)


SHAPE_REFUSALS = [
    (dict(batch=0), b"bad sizes"), (dict(c=0), b"bad sizes"), (dict(batch=-2), b"bad sizes"),
    (dict(h=1), b"at least 2 x 2"), (dict(w=1), b"at least 2 x 2"), (dict(h=0), b"at least 2 x 2"),
    (dict(c=6), b"multiple of 4"), (dict(c=255), b"multiple of 4"),
    (dict(teacher=None), b"null pointer"),
]


@pytest.mark.parametrize("change,message", SHAPE_REFUSALS)
def test_bad_shapes_are_refused_by_name_without_a_gpu(change, message):
    from sgv3d_amd import _lib
    lib = _lib.load()
    calls = [(lambda **k: _warp(lib, False, **k), b"embed_warp:"), (lambda **k: _warp(lib, True, **k), b"embed_warp_host:"),
             (lambda **k: _forward(lib, **k), b"embed_distill_forward:"), (lambda **k: _backward(lib, **k), b"embed_distill_backward:")]
    for call, who in calls:
        assert call(**change) == -1
        err = lib.sgv3d_last_error()
        assert message in err and who in err, err


def test_warp_entries_refuse_null_misaligned_and_overlapping_arguments():
    from sgv3d_amd import _lib
    lib = _lib.load()
    for host, who in ((False, b"embed_warp:"), (True, b"embed_warp_host:")):
        for name in ("minv", "warped", "out"):
            assert _warp(lib, host, **{name: None}) == -1
            assert b"null pointer" in lib.sgv3d_last_error() and who in lib.sgv3d_last_error()
        for out in (P, P + 4 * (4 * 6 * 8) - 16, P - 16):
            assert _warp(lib, host, teacher=P, out=out) == -1 and b"overlaps teacher" in lib.sgv3d_last_error()
    assert _warp(lib, False, teacher=P + 4) == -1 and b"16-byte aligned" in lib.sgv3d_last_error()
    assert _warp(lib, False, out=FAR + 8) == -1 and b"16-byte aligned" in lib.sgv3d_last_error()


def test_distill_entries_refuse_bad_arguments_by_name_without_a_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    for call, who in ((_forward, b"embed_distill_forward:"), (_backward, b"embed_distill_backward:")):
        for change, message in ((dict(student=None), b"null pointer"), (dict(minv=None), b"minv and warped go together"),
                                (dict(warped=None), b"minv and warped go together"), (dict(sc=0), b"bad strides"),
                                (dict(sp=0), b"bad strides"), (dict(sb=-1), b"bad strides"), (dict(sp=-4), b"bad strides"),
                                (dict(teacher=FAR + 4), b"16-byte aligned")):
            assert call(lib, **change) == -1
            err = lib.sgv3d_last_error()
            assert message in err and who in err, err
    for name in ("out", "saved", "ws"):
        assert _forward(lib, **{name: None}) == -1 and b"null pointer" in lib.sgv3d_last_error()
    for weight in (float("nan"), float("inf")):
        assert _forward(lib, weight=weight) == -1 and b"weight must be finite" in lib.sgv3d_last_error()
    assert _forward(lib, ws=P + 4) == -1 and b"8-byte aligned" in lib.sgv3d_last_error()
    for name in ("saved", "grad"):
        assert _backward(lib, **{name: None}) == -1 and b"null pointer" in lib.sgv3d_last_error()
    n = 8 * 4 * 6
    for grad in (FAR, FAR + 4 * n - 4, FAR - 4 * n + 4):                # the gradient view over the teacher, by one element
        assert _backward(lib, grad=grad) == -1 and b"grad overlaps teacher" in lib.sgv3d_last_error()
    # the NHWC view's extent is the same block: strides (C h w, 1, C)
    assert _backward(lib, sc=1, sp=8, grad=FAR - 4 * n + 4) == -1 and b"grad overlaps teacher" in lib.sgv3d_last_error()
    # a batch slice reaches further than its own elements: batch stride twice the frame
    assert _backward(lib, batch=2, sb=2 * n, grad=FAR - 4 * 3 * n + 4) == -1 and b"grad overlaps teacher" in lib.sgv3d_last_error()


def test_short_workspace_is_refused_without_a_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    need = lib.sgv3d_embed_distill_workspace_bytes()
    assert need >= 16 and need % 16 == 0
    assert _forward(lib, nws=need - 1) == -3 and b"workspace too small" in lib.sgv3d_last_error()
    with pytest.raises(_lib.SGV3DError, match="workspace too small"):
        _lib.check(_forward(lib, nws=0), "sgv3d_embed_distill_forward")


# ----------------------------------------------------------------------------------------------- Python layer
def test_coverage_rule():
    from sgv3d_amd import hip_ops
    assert [c for c in range(0, 20) if hip_ops.embed_distill_covers(c, 54, 96)] == [4, 8, 12, 16]
    assert hip_ops.embed_distill_covers(256, 54, 96) and hip_ops.embed_distill_covers(4, 2, 2)
    assert not hip_ops.embed_distill_covers(256, 1, 96) and not hip_ops.embed_distill_covers(256, 54, 1)


def test_the_loss_is_exported_and_keeps_its_defaults():
    import inspect
    import sgv3d_amd.losses as L
    from sgv3d_amd.losses import EmbedDistillation
    assert "EmbedDistillation" in L.__all__ and EmbedDistillation.__module__ == "sgv3d_amd.losses.distill"
    sig = inspect.signature(EmbedDistillation.__init__)
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == dict(
        weight=1000.0, mask_dead=False)
    assert list(inspect.signature(EmbedDistillation.forward).parameters)[1:] == ["assist", "teacher", "minv", "warped"]


def test_cpu_tensors_and_bad_inputs_raise_before_any_launch():
    from sgv3d_amd.distill import warp_embed
    from sgv3d_amd.losses import EmbedDistillation
    with pytest.raises(RuntimeError, match="MI355X only"):
        EmbedDistillation()(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):
        warp_embed(torch.zeros(1, 2, 2, 4), np.eye(3)[None], [1])


def test_sam_teacher_refuses_grids_that_do_not_line_up():
    from sgv3d_amd.distill import SamTeacher
    enc = types.SimpleNamespace(img_size=1024, out_dim=(54, 96))
    t = SamTeacher(enc, dict(final_dim=(864, 1536)))
    assert t.size == (576, 1024) and t.downsample_factor == 16 and abs(t.scale - 0.05) < 1e-15
    with pytest.raises(ValueError, match="crops 576 x 1024"):
        SamTeacher(enc, dict(final_dim=(864, 1536)), src_hw=(1200, 1920))
    with pytest.raises(ValueError, match="whole frame"):                 # bottom crop
        SamTeacher(enc, dict(final_dim=(864, 1536), bot_pct_lim=(0.0, 0.1)))
    with pytest.raises(ValueError, match="whole frame"):                 # another aspect: resize + centre crop
        SamTeacher(types.SimpleNamespace(img_size=1024, out_dim=(54, 80)), dict(final_dim=(864, 1280)))
    with pytest.raises(ValueError, match="out_dim"):
        SamTeacher(types.SimpleNamespace(img_size=1024, out_dim=(54, 95)), dict(final_dim=(864, 1536)))
    with pytest.raises(ValueError, match="out_dim"):
        SamTeacher(types.SimpleNamespace(img_size=1024, out_dim=(108, 96)), dict(final_dim=(864, 1536)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t(torch.zeros(1, 1080, 1920, 3, dtype=torch.uint8))


def test_train_bench_builds_no_distillation_by_default():
    """tools/train_bench.py is a script: its parser's default weight is 0, and everything the distillation builds (the import of
    the loss, the teacher, the model's is_train_height) hangs on that weight being non-zero."""
    tree = ast.parse(open(os.path.join(ROOT, "tools", "train_bench.py")).read())
    defaults = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args:
            kw = {k.arg: k.value for k in node.keywords}
            defaults[node.args[0].value] = (ast.literal_eval(kw["default"]) if "default" in kw else None,
                                            getattr(kw.get("action"), "value", None))
    assert defaults["--distill-weight"] == (0.0, None) and defaults["--distill-mask-dead"] == (None, "store_true")
    flag = [n for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "DISTILL"]
    assert len(flag) == 1 and ast.unparse(flag[0].value) == "args.distill_weight != 0.0"
    guarded = [n for n in tree.body if isinstance(n, ast.If) and ast.unparse(n.test) == "DISTILL"]
    assert len(guarded) == 1
    def names(nodes):
        out = set()
        for top in nodes:
            for n in ast.walk(top):
                out.update(a.name for a in getattr(n, "names", []) if isinstance(a, ast.alias))
                if isinstance(n, ast.Name):
                    out.add(n.id)
                elif isinstance(n, ast.Attribute):
                    out.add(n.attr)
        return out

    inside, outside = names([guarded[0]]), names([n for n in tree.body if n is not guarded[0]])
    for word in ("EmbedDistillation", "SamTeacher", "build_sam_vit_b", "embed_warp_matrices"):
        assert word in inside and word not in outside, word
