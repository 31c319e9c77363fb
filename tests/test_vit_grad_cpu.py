"""Training the SAM ViT encoder, the parts that need no GPU: the C ABI of csrc/vit_grad.hip against its ctypes binding, every
host-side rejection of every new entry, the coverage rule, the float64 restatement of the adjoints (tests/vit_grad_ref.py) against
the gradient fixture and against float64 autograd of tests/vit_ref.py, and the refusals of sgv3d_amd.vit_train."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vit_grad_cases as K
import vit_grad_ref as VG
import vit_ref as V
from conftest import GOLDEN, ROOT

INT_ENTRIES = ("sgv3d_vit_attention_lse", "sgv3d_vit_attention_backward", "sgv3d_layernorm_backward", "sgv3d_gelu_backward",
               "sgv3d_resize_bilinear_backward")
SIZE_ENTRIES = ("sgv3d_vit_attention_backward_workspace_bytes", "sgv3d_layernorm_backward_workspace_bytes")
A = 4096          # a non-null, 16-byte aligned address: every call below is refused before it is looked at


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


def test_attention_lse_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.VitAttnDesc
    call = lambda d, qkv=A, pad=A, rh=A, rw=A, out=A, lse=A: lib.sgv3d_vit_attention_lse(ctypes.byref(d) if d else None, qkv, pad, rh, rw, out, lse, None)
    ok = D(1, 8, 8, 2, 32, 8, 8)
    _rejected(lib, call(ok, lse=None), "null lse")
    _rejected(lib, call(ok, lse=A + 4), "lse must be 16-byte aligned")
    _rejected(lib, call(None), "null descriptor")
    _rejected(lib, call(D(1, 8, 8, 2, 48, 8, 8)), "head_dim")
    _rejected(lib, call(D(1, 8, 0, 2, 32, 8, 8)), "zero or negative dimension")
    _rejected(lib, call(D(1, 8, 8, 2, 32, 129, 8)), "exceeds 128")
    _rejected(lib, call(ok, rh=None), "given together")
    _rejected(lib, call(ok, qkv=None), "null qkv or out")
    _rejected(lib, call(ok, out=A + 8), "16-byte aligned")


def test_attention_backward_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    D = _lib.VitAttnDesc
    names = ("qkv", "pad", "rh", "rw", "out", "lse", "dout", "dqkv", "dpad", "drh", "drw", "ws")

    def call(d, nbytes=None, **kw):
        a = dict.fromkeys(names, A)
        a.update(kw)
        if nbytes is None:
            nbytes = lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(d)) if d else 0
        return lib.sgv3d_vit_attention_backward(ctypes.byref(d) if d else None, *(a[n] for n in names), nbytes, None)

    ok = D(1, 8, 8, 2, 32, 8, 8)
    _rejected(lib, call(None), "null descriptor")
    for hd in (16, 48, 96, 128):
        _rejected(lib, call(D(1, 8, 8, 2, hd, 8, 8)), "head_dim")
    for i in range(7):
        v = [1, 8, 8, 2, 32, 8, 8]
        v[i] = 0
        _rejected(lib, call(D(*v)), "zero or negative dimension")
        assert lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(D(*v))) == 0
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
    _rejected(lib, call(ok, rh=None, rw=None, drh=None), "exactly when the tables are")
    for n in names:
        _rejected(lib, call(ok, **{n: A + 4}), "16-byte aligned")
    # sizes past what the launches can index, refused before the workspace is looked at
    _rejected(lib, call(D(1, 8, 8, 1 << 18, 64, 8, 8)), "heads * head_dim too large")
    assert lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(D(1, 8, 8, 1 << 18, 64, 8, 8))) == 0
    _rejected(lib, call(D(1 << 20, 64, 64, 1, 32, 1, 1)), "too many workgroups")
    _rejected(lib, call(D(1 << 20, 64, 64, 1, 32, 1, 1), rh=None, rw=None, drh=None, drw=None), "too many workgroups")
    # a short or missing workspace: SGV3D_ENOSPACE, before any launch
    need = lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(ok))
    assert need > 0 and need % 16 == 0
    _rejected(lib, call(ok, nbytes=need - 1), "workspace", code=-3)
    _rejected(lib, call(ok, ws=None), "workspace", code=-3)
    # the query and the workspace without tables are allowed to be smaller, never larger
    assert lib.sgv3d_vit_attention_backward_workspace_bytes(ctypes.byref(D(2, 12, 12, 2, 32, 5, 5))) > need


def test_small_kernel_rejections_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    f = ctypes.c_float
    X, DY, DX = 1 << 40, 2 << 40, 3 << 40          # x, dy and dx must not overlap: far apart
    ln = lambda rows=4, c=8, x=X, w=A, eps=1e-6, dy=DY, dx=DX, dw=A, db=A, ws=A, n=1 << 20: lib.sgv3d_layernorm_backward(
        rows, c, x, w, f(eps), dy, dx, dw, db, ws, n, None)
    _rejected(lib, ln(rows=0), "non-positive")
    _rejected(lib, ln(c=0), "non-positive")
    _rejected(lib, ln(c=6), "multiple of 4")
    for n in ("x", "w", "dy", "dx", "dw", "db"):
        _rejected(lib, ln(**{n: None}), "null pointer")
        _rejected(lib, ln(**{n: dict(x=X, dy=DY, dx=DX).get(n, A) + 4}), "16-byte aligned")
    _rejected(lib, ln(ws=A + 8), "16-byte aligned")
    for other in ("x", "dy"):            # 4 rows of 8 floats: 128 bytes each
        _rejected(lib, ln(**{other: DX}), "dx must not overlap x or dy")
        _rejected(lib, ln(**{other: DX + 112}), "dx must not overlap x or dy")
        _rejected(lib, ln(**{other: DX - 112}), "dx must not overlap x or dy")
        assert ln(**{other: DX + 128}, ws=None) == -3 and ln(**{other: DX - 128}, ws=None) == -3       # adjacent is allowed
    _rejected(lib, ln(rows=1 << 33, c=4), "too many rows")
    _rejected(lib, ln(eps=-1.0), "negative eps")
    need = lib.sgv3d_layernorm_backward_workspace_bytes(4097, 1280)
    assert need == 8 * (2 * 4097 + 2 * 129 * 1280)
    assert lib.sgv3d_layernorm_backward_workspace_bytes(0, 8) == 0 and lib.sgv3d_layernorm_backward_workspace_bytes(8, 0) == 0
    _rejected(lib, ln(rows=4097, c=1280, n=need - 1), "workspace", code=-3)
    _rejected(lib, ln(ws=None), "workspace", code=-3)

    _rejected(lib, lib.sgv3d_gelu_backward(0, A, A, A, None), "non-positive")
    _rejected(lib, lib.sgv3d_gelu_backward(1 << 41, A, A, A, None), "too many values")
    for i in (1, 2, 3):
        args = [8, A, A, A, None]
        args[i] = None
        _rejected(lib, lib.sgv3d_gelu_backward(*args), "null pointer")
        args[i] = A + 4
        _rejected(lib, lib.sgv3d_gelu_backward(*args), "16-byte aligned")

    for i in range(8):
        args = [1, 12, 12, 8, 9, 16, 13, 24, A, A, None]
        args[i] = 0
        _rejected(lib, lib.sgv3d_resize_bilinear_backward(*args), "non-positive")
    _rejected(lib, lib.sgv3d_resize_bilinear_backward(1, 12, 12, 6, 9, 16, 13, 24, A, A, None), "multiple of 4")
    _rejected(lib, lib.sgv3d_resize_bilinear_backward(1 << 15, 1 << 15, 1 << 15, 4, 9, 16, 13, 24, A, A, None), "too many pixels")
    _rejected(lib, lib.sgv3d_resize_bilinear_backward(1, 12, 12, 8, 9, 16, 13, 24, None, A, None), "null pointer")
    _rejected(lib, lib.sgv3d_resize_bilinear_backward(1, 12, 12, 8, 9, 16, 13, 24, A, None, None), "null pointer")
    _rejected(lib, lib.sgv3d_resize_bilinear_backward(1, 12, 12, 8, 9, 16, 13, 24, A, A + 8, None), "16-byte aligned")


def test_vit_train_covers():
    from sgv3d_amd.hip_ops import vit_train_covers
    for dim, heads in ((768, 12), (1024, 16), (1280, 16), (64, 2), (32, 1), (80, 1), (240, 3)):
        assert vit_train_covers(dim, heads), (dim, heads)
    for dim, heads in ((96, 2), (64, 4), (128, 1), (64, 3), (0, 1), (64, 0), (-64, 2), (66, 2)):
        assert not vit_train_covers(dim, heads), (dim, heads)


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    base = np.load(os.path.join(GOLDEN, "sam_encoder.npz"))
    return {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith('w/')}, torch.from_numpy(base['input'])


@pytest.mark.parametrize("embed", (False, True), ids=("forward", "embed"))
def test_restatement_matches_the_gradient_fixture(weights, embed):
    """Every parameter gradient of the reference's float64 autograd, to 1e-10 (tensors of 1024 elements or more are stored as a
    float32 head plus a float32 remainder, 48 bits of the float64 value)."""
    wts, img = weights
    fx = VG.open_fixture(GOLDEN, embed)
    got = VG.encoder_backward(wts, V.FIXTURE_CFG, img.double(), torch.from_numpy(fx['cot']).double(), embed=embed)
    assert set(got) == set(wts)
    for name, g in got.items():
        want = VG.fixture_grad(fx, name)
        assert float((g - want).abs().max()) <= 1e-10, name
        assert float(fx[f'ref_f32_grad_err/{name}']) < 1e-3 * float(want.abs().max()), name


def test_fixture_sees_the_four_misreadings(weights):
    wts, img = weights
    fx = VG.open_fixture(GOLDEN)
    cot = torch.from_numpy(fx['cot']).double()
    for kw, name in ((dict(pad_bias=False), 'blocks.0.attn.qkv.bias'), (dict(rel_in_dq=False), 'blocks.1.attn.qkv.weight'),
                     (dict(rel_scaled_q=True), 'blocks.1.attn.rel_pos_h'), (dict(pad_queries=True), 'blocks.0.attn.qkv.weight')):
        want = VG.fixture_grad(fx, name)
        wrong = VG.encoder_backward(wts, V.FIXTURE_CFG, img.double(), cot, **kw)[name]
        bar = max(4.0 * float(fx[f'ref_f32_grad_err/{name}']), 2.0 ** -21 * float(want.abs().max()))
        assert float((wrong - want).abs().max()) > 100.0 * bar, kw


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_attention_restatement_against_autograd(i):
    """The written-out backward against float64 autograd of tests/vit_ref.py's attention on the kernel-test shapes."""
    c = K.CASES[i]
    leaves = [None if t is None else t.double().requires_grad_() for t in K.inputs(i)[:4]]
    dout = K.inputs(i)[4].double()
    out = V.attention(leaves[0], c['heads'], c['window'], *leaves[1:])
    grads = torch.autograd.grad((out * dout).sum(), [t for t in leaves if t is not None], allow_unused=True)
    it = iter(grads)
    auto = [None if t is None else next(it) for t in leaves]
    mine = K.reference(i)
    assert float((mine['out'] - out.detach()).abs().max()) <= 1e-12
    for key, g in zip(('dqkv', 'dpad', 'drh', 'drw'), auto):
        if g is not None:
            assert float((mine[key] - g).abs().max()) <= 1e-10 * max(1.0, float(g.abs().max())), key
    if c['pad']:
        assert float(mine['dpad'][:c['heads'] * c['head_dim']].abs().max()) == 0.0


def test_small_restatements_against_autograd():
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(7, 36, generator=g, dtype=torch.float64) + 3.0).requires_grad_()
    w = torch.randn(36, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(36, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(7, 36, generator=g, dtype=torch.float64)
    auto = torch.autograd.grad((V.layernorm(x, w, b, 1e-6) * dy).sum(), (x, w, b))
    for got, want in zip(VG.layernorm_backward(x.detach(), w.detach(), 1e-6, dy), auto):
        assert float((got - want).abs().max()) <= 1e-10
    x = torch.linspace(-12, 12, 97, dtype=torch.float64).requires_grad_()
    auto, = torch.autograd.grad(V.gelu(x).sum(), x)
    assert float((VG.gelu_backward(x.detach(), torch.ones_like(x)) - auto).abs().max()) <= 1e-14
    for hw, crop, size in (((12, 12), (9, 16), (13, 24)), ((12, 10), (12, 10), (5, 3)), ((6, 7), (4, 5), (9, 11))):
        x = torch.randn(2, *hw, 4, generator=g, dtype=torch.float64).requires_grad_()
        dy = torch.randn(2, *size, 4, generator=g, dtype=torch.float64)
        auto, = torch.autograd.grad((V.resize_bilinear(x, crop, size) * dy).sum(), x)
        assert float((VG.resize_bilinear_backward(dy, hw, crop) - auto).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------
def test_vit_train_refusals():
    from sgv3d_amd import vit_train
    from sgv3d_amd._lib import SGV3DError
    from sgv3d_amd.layers.backbones.sam_encoder import Attention, Block, ImageEncoderViT
    enc = ImageEncoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, out_chans=8)
    for fn in (vit_train.encoder_forward, vit_train.encoder_embed):
        with pytest.raises(SGV3DError, match="the image x requires grad"):
            fn(enc, torch.zeros(1, 3, 32, 32, requires_grad=True))
        with pytest.raises(SGV3DError, match="no CPU fallback"):
            fn(enc, torch.zeros(1, 3, 32, 32))
        with pytest.raises(SGV3DError, match="a tensor is expected"):
            fn(enc, None)
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        vit_train.block_forward(Block(64, 2), torch.zeros(1, 4, 4, 64))
    with pytest.raises(SGV3DError, match="no CPU fallback"):
        vit_train.attention_forward(Attention(64, 2), torch.zeros(1, 4, 4, 64))


def test_the_modules_stay_inference_only():
    from sgv3d_amd._lib import SGV3DError
    from sgv3d_amd.layers.backbones.sam_encoder import Attention, Block, ImageEncoderViT
    enc = ImageEncoderViT(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, out_chans=8)
    for call in (lambda: enc(torch.zeros(1, 3, 32, 32, requires_grad=True)), lambda: enc.embed(torch.zeros(1, 3, 32, 32, requires_grad=True)),
                 lambda: Block(64, 2)(torch.zeros(1, 4, 4, 64, requires_grad=True)),
                 lambda: Attention(64, 2)(torch.zeros(1, 4, 4, 64, requires_grad=True))):
        with pytest.raises(SGV3DError, match="inference only: the input requires grad"):
            call()
