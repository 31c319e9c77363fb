"""Training the SAM ViT encoder in bf16 mode, the parts that need no GPU: the C ABI of the new entries against their ctypes binding,
every host-side rejection of every new entry, the activation rule of hip_ops.VIT_TRAIN_BF16, the restatement with the rounding points
off against tests/vit_grad_ref.py, the fixture, and what sgv3d_amd.vit_train asks of its layers with the switch off and on."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import vit_grad_bf16_ref as R
import vit_grad_cases as K
import vit_grad_ref as VG
import vit_ref as V
from conftest import GOLDEN, ROOT

INT_ENTRIES = ("sgv3d_vit_attention_bf16_lse", "sgv3d_vit_attention_bf16_backward", "sgv3d_layernorm_backward_bf16dy",
               "sgv3d_gelu_backward_bf16")
SIZE_ENTRIES = ("sgv3d_vit_attention_bf16_backward_workspace_bytes",)
A = 4096          # a non-null, 16-byte aligned address: every call below is refused before it is looked at
FAR = 1 << 40     # tensors that must not overlap sit this far apart


def _ctype_of(decl):
    if "*" in decl:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[decl.rsplit(" ", 1)[0]]


def test_header_matches_ctypes():
    from sgv3d_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read(), flags=re.S)
    for names, ret, res in ((INT_ENTRIES, "int", ctypes.c_int), (SIZE_ENTRIES, "size_t", ctypes.c_size_t)):
        for name in names:
            m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
            assert m, f"{name} is not declared in sgv3d_hip.h"
            args = [" ".join(a.split()) for a in m.group(1).split(",")]
            got_res, argtypes = _lib._PROTOS[name]
            assert got_res is res
            got = [ctypes.c_void_p if (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t for t in argtypes]
            assert got == [_ctype_of(a) for a in args], f"{name}: ctypes {got} against the header's {args}"
            assert name in _lib.EXPORTED_SYMBOLS


def _rejected(lib, rc, word, code=-1):
    msg = lib.sgv3d_last_error().decode()
    assert rc == code and word in msg, (rc, msg)


def test_attention_bf16_lse_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.VitAttnDesc
    call = lambda d, qkv=A, pad=A, rh=A, rw=A, out=A, lse=A: lib.sgv3d_vit_attention_bf16_lse(ctypes.byref(d) if d else None, qkv, pad, rh, rw, out, lse, None)
    ok = D(1, 8, 8, 2, 32, 8, 8)
    _rejected(lib, call(ok, lse=None), "null lse")
    _rejected(lib, call(ok, lse=A + 4), "lse must be 16-byte aligned")
    _rejected(lib, call(None), "vit_attention_bf16_lse: null descriptor")
    for hd in (16, 48, 96, 128):
        _rejected(lib, call(D(1, 8, 8, 2, hd, 8, 8)), "head_dim")
    _rejected(lib, call(D(1, 8, 0, 2, 32, 8, 8)), "zero or negative dimension")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 129, 8)), "exceeds 128")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 0)), "zero or negative dimension")
    _rejected(lib, call(ok, rh=None), "given together")
    _rejected(lib, call(ok, qkv=None), "vit_attention_bf16_lse: null qkv or out")
    _rejected(lib, call(ok, out=None), "null qkv or out")
    for n in ("qkv", "pad", "rh", "rw", "out"):
        _rejected(lib, call(ok, **{n: A + 8}), "16-byte aligned")
    # the entry without lse keeps its own name in its messages
    assert lib.sgv3d_vit_attention_bf16(ctypes.byref(ok), None, A, A, A, A, None) == -1
    assert b"vit_attention_bf16: null qkv or out" in lib.sgv3d_last_error()


def test_attention_bf16_backward_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.VitAttnDesc
    names = ("qkv", "pad", "rh", "rw", "out", "lse", "dout", "dqkv", "dpad", "drh", "drw", "ws")
    far = dict(qkv=FAR, out=2 * FAR, dout=3 * FAR, dqkv=4 * FAR)

    def call(d, nbytes=None, **kw):
        a = dict.fromkeys(names, A)
        a.update(far)
        a.update(kw)
        if nbytes is None:
            nbytes = lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(d)) if d else 0
        return lib.sgv3d_vit_attention_bf16_backward(ctypes.byref(d) if d else None, *(a[n] for n in names), nbytes, None)

    ok = D(1, 8, 8, 2, 32, 8, 8)
    _rejected(lib, call(None), "null descriptor")
    for hd in (16, 48, 96, 128):
        _rejected(lib, call(D(1, 8, 8, 2, hd, 8, 8)), "head_dim")
        assert lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(D(1, 8, 8, 2, hd, 8, 8))) == 0
    for i in range(7):
        v = [1, 8, 8, 2, 32, 8, 8]
        v[i] = 0
        _rejected(lib, call(D(*v)), "zero or negative dimension")
        assert lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(D(*v))) == 0
    _rejected(lib, call(D(1, 8, 8, 2, 32, 129, 8)), "exceeds 128")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 8, 129)), "exceeds 128")
    _rejected(lib, call(ok, rh=None), "given together")
    _rejected(lib, call(ok, rw=None), "given together")
    for n in ("qkv", "out", "lse", "dout", "dqkv"):
        _rejected(lib, call(ok, **{n: None}), "null qkv, out, lse, dout or dqkv")
    _rejected(lib, call(ok, dpad=None), "dpad_qkv is null")
    _rejected(lib, call(ok, drh=None), "exactly when the tables are")
    _rejected(lib, call(ok, drw=None), "exactly when the tables are")
    _rejected(lib, call(ok, rh=None, rw=None), "exactly when the tables are")
    for n in names:
        _rejected(lib, call(ok, **{n: far.get(n, A) + 4}), "16-byte aligned")
    # dqkv [1, 8, 8, 192] bf16 is 24 576 bytes, out and dout 8 192: on top of, or reaching into, a tensor the launches still read
    for other, span in (("qkv", 24576), ("out", 8192), ("dout", 8192)):
        _rejected(lib, call(ok, **{other: far["dqkv"]}), "dqkv must not overlap qkv, out or dout")
        _rejected(lib, call(ok, **{other: far["dqkv"] + 24576 - 16}), "dqkv must not overlap")
        _rejected(lib, call(ok, **{other: far["dqkv"] - span + 16}), "dqkv must not overlap")
        assert call(ok, **{other: far["dqkv"] + 24576}, ws=None) == -3 and call(ok, **{other: far["dqkv"] - span}, ws=None) == -3     # adjacent is allowed
    _rejected(lib, call(D(1, 8, 8, 1 << 18, 64, 8, 8)), "heads * head_dim too large")
    _rejected(lib, call(D(1 << 20, 64, 64, 1, 32, 1, 1)), "too many workgroups")
    # a short or missing workspace: SGV3D_ENOSPACE, before any launch
    need = lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(ok))
    assert need > 0 and need % 16 == 0
    _rejected(lib, call(ok, nbytes=need - 1), "workspace", code=-3)
    _rejected(lib, call(ok, ws=None), "workspace", code=-3)
    assert lib.sgv3d_vit_attention_bf16_backward_workspace_bytes(ctypes.byref(D(2, 12, 12, 2, 32, 5, 5))) > need


def test_thin_entry_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float
    X, DY, DX = FAR, 2 * FAR, 3 * FAR
    ln = lambda rows=4, c=8, x=X, w=A, eps=1e-6, dy=DY, dx=DX, dw=A, db=A, ws=A, n=1 << 20: lib.sgv3d_layernorm_backward_bf16dy(
        rows, c, x, w, f(eps), dy, dx, dw, db, ws, n, None)
    _rejected(lib, ln(rows=0), "layernorm_backward_bf16dy: non-positive")
    _rejected(lib, ln(c=0), "non-positive")
    _rejected(lib, ln(c=6), "multiple of 4")
    for n in ("x", "w", "dy", "dx", "dw", "db"):
        _rejected(lib, ln(**{n: None}), "null pointer")
        _rejected(lib, ln(**{n: dict(x=X, dy=DY, dx=DX).get(n, A) + 4}), "16-byte aligned")
    _rejected(lib, ln(ws=A + 8), "16-byte aligned")
    for other in ("x", "dy"):
        _rejected(lib, ln(**{other: DX}), "dx must not overlap x or dy")
        _rejected(lib, ln(**{other: DX + 112}), "dx must not overlap x or dy")
    _rejected(lib, ln(rows=1 << 33, c=4), "too many rows")
    _rejected(lib, ln(eps=-1.0), "negative eps")
    need = lib.sgv3d_layernorm_backward_workspace_bytes(4097, 1280)
    _rejected(lib, ln(rows=4097, c=1280, n=need - 1), "workspace", code=-3)
    _rejected(lib, ln(ws=None), "workspace", code=-3)

    ge = lambda n=64, x=X, dy=DY, dx=DX: lib.sgv3d_gelu_backward_bf16(n, x, dy, dx, None)
    _rejected(lib, ge(n=0), "non-positive")
    _rejected(lib, ge(n=1 << 42, x=A, dy=A, dx=A), "too many values")         # (in place: 8 TiB tensors cannot sit apart)
    for name, addr in (("x", X), ("dy", DY), ("dx", DX)):
        _rejected(lib, ge(**{name: None}), "null pointer")
        _rejected(lib, ge(**{name: addr + 8}), "16-byte aligned")
    # 64 bf16 values are 128 bytes: a shifted overlap is refused, the tensor itself (in place) is not looked at further here
    _rejected(lib, ge(dx=X + 16), "dx must be x, dy or a tensor that overlaps neither")
    _rejected(lib, ge(dx=DY - 112), "dx must be x, dy or a tensor that overlaps neither")


def test_activation_rule_in_every_combination():
    from sgv3d_amd import hip_ops
    saved = {k: getattr(hip_ops, k) for k in ("VIT_TRAIN_BF16", "MFMA_BF16", "MFMA_F32X3", "TRAIN_BF16_WGRAD")}
    try:
        for switch, bf16, x3, wgrad in itertools.product((False, True), (False, True), (False, True, "auto"), (False, True)):
            hip_ops.VIT_TRAIN_BF16, hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.TRAIN_BF16_WGRAD = switch, bf16, x3, wgrad
            want = switch and bf16 and not x3 and wgrad
            assert hip_ops.vit_train_bf16_active(768, 12, 3072) is bool(want)
            assert hip_ops.vit_train_bf16_active(64, 2) is bool(want)
            # a Block the bf16 kernels do not take (rows that are no multiple of 16 bytes, a head_dim outside 32 / 64 / 80): never
            for dim, heads, mlp in ((768, 12, 3076), (36, 1, 144), (96, 2, 384), (64, 3, 256), (0, 1, 8)):
                assert hip_ops.vit_train_bf16_active(dim, heads, mlp) is False
    finally:
        for k, v in saved.items():
            setattr(hip_ops, k, v)
    assert saved["VIT_TRAIN_BF16"] == (os.environ.get("SGV3D_VIT_TRAIN_BF16", "0") not in ("", "0")), "off by default"


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_restatement_with_rounding_off_is_vit_grad_ref(i):
    c = K.CASES[i]
    args = [None if t is None else t.double() for t in K.inputs(i)]
    want = K.reference(i)
    out, lse = R.attention_forward(args[0], c['heads'], c['window'], *args[1:4])
    assert float((out - want['out']).abs().max()) <= 1e-12 and float((lse - want['lse']).abs().max()) <= 1e-12
    got = R.attention_backward(args[0], c['heads'], c['window'], *args[1:4], args[4])
    for key, g in zip(('dqkv', 'dpad', 'drh', 'drw'), got):
        if g is not None:
            assert float((g - want[key]).abs().max()) <= 1e-12 * max(1.0, float(want[key].abs().max())), key


def test_restatement_rounding_points_move_the_result_a_little():
    """Each switch alone changes the gradients, by an amount of the size of its rounding (bf16: 2^-9 relative)."""
    i = 0
    c = K.CASES[i]
    qkv, pad, rh, rw, dout = (None if t is None else t.double() for t in K.inputs(i))
    qkv, dout = R.bf16(qkv), R.bf16(dout)
    base = R.attention_backward(qkv, c['heads'], c['window'], pad, rh, rw, dout)
    for kw in (dict(operands=True), dict(p_ds=True), dict(f32_sums=True), R.ALL_ON):
        got = R.attention_backward(qkv, c['heads'], c['window'], pad, rh, rw, dout, **kw)
        rel = float((got[0] - base[0]).norm() / base[0].norm())
        assert 0.0 < rel < 2.0 ** -5, (kw, rel)
    assert R.bf16(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)).tolist() == [1.0, 1.0 + 2.0 ** -6]     # ties to even


def test_fixture_is_present_and_whole():
    fx = np.load(os.path.join(GOLDEN, "sam_encoder_grad_bf16.npz"))
    base = np.load(os.path.join(GOLDEN, "sam_encoder.npz"))
    names = [k[2:] for k in base.files if k.startswith('w/')]
    assert len(names) == 37
    assert sorted(fx.files) == sorted(f"{run}/{what}/{n}" for run in ("forward", "embed") for what in ("max_abs", "rel_l2") for n in names)
    for k in fx.files:
        assert fx[k].shape == () and fx[k].dtype == np.float64 and np.isfinite(fx[k]) and fx[k] >= 0.0
    rel = sorted(float(fx[f"forward/rel_l2/{n}"]) for n in names)
    assert 1e-3 < rel[len(rel) // 2] < 2e-2 and rel[-1] < 4e-2, "the reference's own bf16 error is of the size of bf16 rounding"
    assert os.path.getsize(os.path.join(GOLDEN, "sam_encoder_grad_bf16.npz")) < 1000000


def test_the_modules_stay_inference_only(monkeypatch):
    from sgv3d_amd import hip_ops
    from sgv3d_amd._lib import SGV3DError
    from sgv3d_amd.layers.backbones.sam_encoder import Attention, Block, ImageEncoderViT
    for k in ("VIT_TRAIN_BF16", "MFMA_BF16", "TRAIN_BF16_WGRAD"):
        monkeypatch.setattr(hip_ops, k, True)
    monkeypatch.setattr(hip_ops, "MFMA_F32X3", False)
    enc = ImageEncoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, out_chans=8)
    for call in (lambda: enc(torch.zeros(1, 3, 32, 32, requires_grad=True)), lambda: enc.embed(torch.zeros(1, 3, 32, 32, requires_grad=True)),
                 lambda: Block(64, 2)(torch.zeros(1, 4, 4, 64, requires_grad=True)),
                 lambda: Attention(64, 2)(torch.zeros(1, 4, 4, 64, requires_grad=True))):
        with pytest.raises(SGV3DError, match="inference only: the input requires grad"):
            call()
    assert not Block(64, 2).bf16_mode(), "the module forward's bf16 mode is hip_ops.VIT_BF16's, not the training switch's"


@pytest.mark.parametrize("switch", (False, True), ids=("off", "on"))
def test_what_block_forward_asks_of_its_layers(monkeypatch, switch):
    """Stand-ins for the device layers record the dtypes block_forward asks for.  Switch off: no bf16 anywhere, every call as
    before (no out_dtype argument reaches a layer).  On: LayerNorm -> bf16, qkv and lin1 bf16 -> bf16, proj and lin2 bf16 -> f32."""
    from sgv3d_amd import hip_ops, vit_grad, vit_train
    from sgv3d_amd.layers.backbones.sam_encoder import Block
    monkeypatch.setattr(hip_ops, "MFMA_BF16", True)
    monkeypatch.setattr(hip_ops, "MFMA_F32X3", False)
    monkeypatch.setattr(hip_ops, "TRAIN_BF16_WGRAD", True)
    monkeypatch.setattr(hip_ops, "VIT_TRAIN_BF16", switch)
    monkeypatch.setattr(hip_ops, "VIT_BF16", True)           # the inference switch has no say in training
    log = []
    monkeypatch.setattr(vit_train, "_require", lambda *a, **k: None)

    def layer_norm(x, w, b, eps, *rest, **kw):
        log.append(("layer_norm", x.dtype, rest, kw))
        return x.to(kw.get("out_dtype") or x.dtype)

    def packed_apply(x, weight, bias, residual, packed, kw, *rest):
        log.append(("packed", x.dtype, rest))
        return torch.zeros(*x.shape[:-1], weight.shape[0], dtype=(rest[0] if rest else torch.float32))
    monkeypatch.setattr(vit_grad, "layer_norm", layer_norm)
    monkeypatch.setattr(vit_grad, "gelu", lambda x: (log.append(("gelu", x.dtype)), x)[1])
    monkeypatch.setattr(vit_grad, "attention", lambda qkv, *a: (log.append(("attention", qkv.dtype)), qkv[..., :qkv.shape[-1] // 3])[1])
    monkeypatch.setattr(vit_train._PackedLayer, "apply", packed_apply)
    out = vit_train.block_forward(Block(64, 2), torch.zeros(1, 4, 4, 64))
    assert out.dtype == torch.float32
    f32, bf = torch.float32, torch.bfloat16
    if switch:
        assert log == [("layer_norm", f32, (), dict(out_dtype=bf)), ("packed", bf, (bf,)), ("attention", bf), ("packed", bf, ()),
                       ("layer_norm", f32, (), dict(out_dtype=bf)), ("packed", bf, (bf,)), ("gelu", bf), ("packed", bf, ())]
    else:
        assert log == [("layer_norm", f32, (), dict(out_dtype=None)), ("packed", f32, ()), ("attention", f32), ("packed", f32, ()),
                       ("layer_norm", f32, (), dict(out_dtype=None)), ("packed", f32, ()), ("gelu", f32), ("packed", f32, ())]


def test_vit_grad_dispatch_without_the_switch_names_only_f32_entries(monkeypatch):
    """vit_grad's wrappers pick an entry by the dtype of the tensors alone: f32 tensors never reach a bf16 entry."""
    from sgv3d_amd import _lib, vit_grad
    called = []

    class Lib:
        def __getattr__(self, name):
            def entry(*a):
                called.append(name)
                return 0
            return entry
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(_lib, "stream_handle", lambda dev: None)
    monkeypatch.setattr(vit_grad, "_f32", lambda *t: None)
    monkeypatch.setattr(vit_grad, "_bf16", lambda *t: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    for dt, sfx in ((torch.float32, ""), (torch.bfloat16, "_bf16")):
        called.clear()
        x, dy = torch.zeros(2, 8, dtype=dt), torch.zeros(2, 8, dtype=dt)
        vit_grad.gelu_backward(x, dy)
        vit_grad.layernorm_backward(torch.zeros(2, 8), torch.ones(8), 1e-6, dy)
        qkv = torch.zeros(1, 2, 2, 96, dtype=dt)
        out, lse = vit_grad.attention_lse(qkv, 1, (2, 2))
        vit_grad.attention_backward(qkv, 1, (2, 2), None, None, None, out, lse, out)
        assert called == ["sgv3d_gelu_backward" + sfx, "sgv3d_layernorm_backward_workspace_bytes",
                          "sgv3d_layernorm_backward" + ("_bf16dy" if sfx else ""), f"sgv3d_vit_attention{sfx}_lse",
                          f"sgv3d_vit_attention{sfx}_backward_workspace_bytes", f"sgv3d_vit_attention{sfx}_backward"]
