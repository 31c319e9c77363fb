"""The forward convolution kernels at the layer geometries only the data gradient builds -- non-square kernels, padding beyond the
kernel's reach, dilation beyond the map -- with every eligible tile forced, and conv_grad.conv2d's forward / data gradient / weight
gradient end to end over small kernels, strides, paddings and maps.  Dyadic data (conv_geometry.py): the float64 reference is the
exact expected output in f32, f32x3 and bf16 mode, so every comparison is ``torch.equal``."""
import functools

import pytest
import torch

import conv_geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture
def ops(monkeypatch):
    """hip_ops with its mode switches restored afterwards; f32 mode, no first-call timing unless the test says otherwise."""
    from sgv3d_amd import hip_ops
    for name, value in (("MFMA_BF16", False), ("MFMA_F32X3", False), ("BF16_ACTIVATIONS", False), ("AUTOTUNE", False)):
        monkeypatch.setattr(hip_ops, name, value)
    return hip_ops


def _set_mode(monkeypatch, ops, mode):
    monkeypatch.setattr(ops, "MFMA_BF16", mode in ("bf16", "bf16io"))
    monkeypatch.setattr(ops, "MFMA_F32X3", mode == "f32x3")


# ============================================================================================ (a) forward PackedConv, tiles forced
# (cin, cout, (kh, kw), stride, pad, dil, B, H, W)
LISTED = [
    (64, 64, (2, 1), 1, 1, 1, 2, 8, 11),      # a one-tap axis with padding 1: first and last output columns are pure padding
    (64, 64, (1, 2), 1, 1, 1, 2, 8, 11),      # ... rows
    (64, 64, (2, 1), 1, 2, 1, 1, 9, 70),      # output rows wider than a 64-row m-tile: the first tile has no valid kernel row, the second one
    (64, 96, (1, 1), 1, 1, 1, 1, 9, 70),      # 1x1 WITH padding: not the pointwise / plain instantiation
    (64, 64, (4, 3), 1, 3, 1, 2, 6, 9),       # the 7x7 stem's phases
    (64, 64, (3, 4), 1, 3, 1, 2, 6, 9),
    (32, 36, (3, 2), 1, 2, 1, 3, 5, 7),       # FAST path below the pw_x3 channel floor; cout % 8 != 0; m-tiles that span images
    (12, 8, (3, 4), 1, 2, 1, 1, 7, 6),        # tap-major k (cin % 32 != 0), taps * cin >= 128: the TM form of conv_pw_x3
    (64, 64, (3, 3), 1, 12, 12, 1, 7, 9),     # dilation beyond the map, one 64-row tile (7 * 9 = 63)
    (64, 64, (3, 3), 1, 18, 18, 2, 21, 5),    # ... tiles that span two images
    (64, 64, (3, 3), 1, 6, 6, 1, 14, 66),     # one-row tiles whose valid kernel-row range differs from tile to tile
    (64, 64, (3, 2), 2, 1, 2, 2, 9, 12),      # non-square with stride and dilation together
    (64, 32, (1, 5), 1, 2, 1, 1, 6, 10),      # 1x5 with padding
]


def _forms():
    forms = [G.Form(cin, cout, kh, kw, s, p, d, H, W, f"b{B}") for cin, cout, (kh, kw), s, p, d, B, H, W in LISTED]
    # what the stride-2 data gradient builds for the 3x3 and 7x7 layers at pad 0, 1 and 3 on maps of both parities
    for k in (3, 7):
        for pad in (0, 1, 3):
            for H, W in ((10, 13), (11, 12)):
                for f in G.dgrad_forms(k, 2, pad, 1, H, W, 64, 64):
                    f = f._replace(kind="b2")
                    if f not in forms:
                        forms.append(f)
    return forms


FORMS = _forms()
_form_id = lambda f: f"{f.cin}-{f.cout}-k{f.kh}x{f.kw}-s{f.stride}p{f.pad}d{f.dil}-{f.kind}x{f.H}x{f.W}"
MODES = ("f32", "f32x3", "bf16", "bf16io")


@functools.lru_cache(maxsize=None)
def _form_case(f):
    """Data and exact references of one form, made once on the CPU: the activations sit at channel offset 4 (f32) / 8 (bf16) of a wider
    tensor whose other channels are not zero."""
    g = torch.Generator().manual_seed(hash(tuple(f[:9])) & 0xffff)
    B = int(f.kind[1:])
    assert f.cin * f.kh * f.kw <= G.K_MAX
    G.assert_exact(f.cin * f.kh * f.kw)
    wide = G.dyadic((B, f.H, f.W, f.cin + 16), 8, g)
    w = G.dyadic((f.cout, f.cin, f.kh, f.kw), 4, g)
    oh, ow = G.out_hw(f.H, f.W, f.kh, f.kw, f.stride, f.pad, f.dil)
    scale, shift = G.epilogue(f.cout, g)
    res = G.dyadic((B, oh, ow, f.cout), 8, g)
    case = dict(w=w, scale=scale, shift=shift, res=res, wide=wide, ohw=(oh, ow), B=B)
    for coff in (4, 8):
        x = wide[..., coff:coff + f.cin]
        if f.kh != f.kw:
            plain = G.assert_discriminates(x, w, f.stride, f.pad, f.dil)
        else:
            plain = G.conv_ref(x, w, f.stride, f.pad, f.dil)
        full = G.conv_ref(x, w, f.stride, f.pad, f.dil, scale, shift, res, relu=True)
        for r in (plain, full):
            assert torch.equal(r.float().double(), r)                  # the reference IS an f32 value
        assert float(plain.abs().max()) > 0 and float(full.max()) > 0
        case[coff] = (plain, full)
    return case


def _tiles(ops, conv, f, mode):
    """(tile, splits) pairs of a form in a mode, by the project's own predicates."""
    from sgv3d_amd.conv_tiles import TILES, select
    nk_igemm = conv.k_pad // 32
    splits = lambda nk: tuple(s for s in (1, 2, 3) if s <= nk)
    if mode == "f32":
        tiles = list(select("igemm")) + [t for t in select("igemm", mfirst=True) if f.cout > TILES[t].bn]
        if conv.k_order == 1:
            tiles += list(ops.OCC5_TILES)
        out = [(t, splits(nk_igemm)) for t in tiles]
        if conv.pw_x3_ok():
            out += [(t, splits((f.cin * f.kh * f.kw + 31) // 32)) for t in ops.PW_X3_TILES if TILES[t].bn < 256 or f.cout >= 256]
        return out
    if mode == "f32x3":
        return [(t, splits(nk_igemm)) for t in select("igemm") + select("igemm", mfirst=True)]
    out = [(t, splits(nk_igemm)) for t in select("igemm")]
    if mode == "bf16io" and f.cin % 32 == 0 and f.cout % 8 == 0:
        nk_dw = -(-(f.kh * f.kw * (f.cin // 32)) // 2)               # chunks of 64 k: what the split-K entry accepts
        out += [(t, (1,) if TILES[t].deep else splits(nk_dw)) for t in range(31, 40)]
    return out


# (bf16 tensors in and out: 16-byte pixel rows, channel counts % 8 -- the other forms have no such launch)
FORM_MODES = [pytest.param(f, mode, id=f"{_form_id(f)}-{mode}") for f in FORMS for mode in MODES
              if mode != "bf16io" or (f.cin % 8 == 0 and f.cout % 8 == 0)]


@pytest.mark.parametrize("f,mode", FORM_MODES)
def test_forward_every_tile_is_exact(ops, monkeypatch, f, mode):
    from sgv3d_amd.hip_ops import PackedConv
    io = mode == "bf16io"
    case = _form_case(f)
    coff = 8 if io else 4
    dt = torch.bfloat16 if io else torch.float32
    B, (oh, ow) = case["B"], case["ohw"]
    xw = case["wide"][..., :f.cin + 2 * coff].contiguous().to(dt).cuda()
    res = case["res"].to(dt).cuda()
    w = case["w"].cuda()
    want = [r.float().to(dt).cuda() for r in case[coff]]              # (bf16 output: the exact value rounded once)
    _set_mode(monkeypatch, ops, "f32")
    probe = PackedConv(w, stride=f.stride, pad=f.pad, dil=f.dil)
    pairs = _tiles(ops, probe, f, mode)                               # (pw_x3_ok is a statement about f32 mode)
    _set_mode(monkeypatch, ops, mode)
    convs = (PackedConv(w, stride=f.stride, pad=f.pad, dil=f.dil),
             PackedConv(w, stride=f.stride, pad=f.pad, dil=f.dil, scale=case["scale"].cuda(), shift=case["shift"].cuda(), relu=True))
    n = 0
    for epi, conv in enumerate(convs):
        for t, splits in pairs:
            for s in splits:
                outs = []
                for _ in range(2):
                    out = torch.full((B, oh, ow, f.cout + 2 * coff), -7.0, dtype=dt, device="cuda")
                    conv(xw, out, x_coff=coff, y_coff=coff, residual=res if epi else None, tile=t, split_k=s)
                    outs.append(out)
                got = outs[0]
                assert torch.equal(got[..., coff:coff + f.cout], want[epi]), (t, s, epi)
                assert bool((got[..., :coff] == -7).all()) and bool((got[..., coff + f.cout:] == -7).all()), (t, s, epi, "guard channels")
                assert torch.equal(outs[0], outs[1]), (t, s, epi, "second launch")
                n += 1
    assert n >= 2 * len(pairs)
    print(f"[conv-geometry] forward {_form_id(f)} {mode}: {n} (tile, split, epilogue) combinations exact")


def test_forward_forms_reach_the_paths_they_are_for(ops):
    """The tile lists are not empty where the forms were chosen for a kernel family."""
    from sgv3d_amd.hip_ops import PackedConv
    by = {_form_id(f): f for f in FORMS}
    probe = lambda f: PackedConv(torch.zeros(f.cout, f.cin, f.kh, f.kw, device="cuda"), stride=f.stride, pad=f.pad, dil=f.dil)
    fam = lambda f, mode: {ops.TILES[t].family + ("_occ5" if ops.TILES[t].occ5 else "") for t, _ in _tiles(ops, probe(f), f, mode)}
    tm = by["12-8-k3x4-s1p2d1-b1x7x6"]
    assert probe(tm).k_order == 0 and "pw_x3" in fam(tm, "f32") and "igemm_occ5" not in fam(tm, "f32")
    low = by["32-36-k3x2-s1p2d1-b3x5x7"]
    assert probe(low).k_order == 1 and "pw_x3" not in fam(low, "f32") and "igemm_occ5" in fam(low, "f32")
    one = by["64-96-k1x1-s1p1d1-b1x9x70"]
    assert {"pw_x3", "igemm_occ5", "igemm"} <= fam(one, "f32") and "dw_bf16" in fam(one, "bf16io")
    stem = by["64-64-k4x3-s1p3d1-b2x6x9"]
    assert any(s == (1, 2, 3) for _, s in _tiles(ops, probe(stem), stem, "bf16io")[4:])    # the direct-weight split-K entry


# ===================================================================================== (b) conv_grad.conv2d and its backward
KS = [(k, s) for k in (1, 2, 3, 4, 5, 7) for s in (1, 2, 3)]
MAPS = ((1, 1), (2, 3), (5, 4), (6, 7), (9, 8))
BATCH = 2


def _geoms(k, stride):
    for pad in sorted({0, k // 2, k - 1}):
        for dil in ((1, 2) if k == 3 else (1,)):
            for H, W in MAPS:
                oh, ow = G.out_hw(H, W, k, k, stride, pad, dil)
                if oh > 0 and ow > 0 and pad <= dil * (k - 1):
                    yield pad, dil, H, W


@functools.lru_cache(maxsize=None)
def _grad_cases(k, stride, cin, cout):
    """[(pad, dil, H, W, x, w, dy, y, dx, dw)] of one (kernel, stride, channels): data and float64 autograd, made once."""
    g = torch.Generator().manual_seed(1000 * k + 100 * stride + cin + cout)
    out = []
    for pad, dil, H, W in _geoms(k, stride):
        oh, ow = G.out_hw(H, W, k, k, stride, pad, dil)
        G.assert_exact(max(cin, (cout + 3) // 4 * 4) * k * k)         # y and dx: products of magnitude <= 2
        G.assert_exact(BATCH * oh * ow, max_product=4.0)              # dw: x * dy
        x, w, dy = G.dyadic((BATCH, H, W, cin), 8, g), G.dyadic((cout, cin, k, k), 4, g), G.dyadic((BATCH, oh, ow, cout), 8, g)
        y, dx, dw = G.autograd_reference(x, w, dy, stride, pad, dil)
        for r in (y, dx, dw):
            assert torch.equal(r.float().double(), r)
        out.append((pad, dil, H, W, x, w, dy, y, dx, dw))
    assert out
    return out


def _run_grad(k, stride, cin, cout, dtype=torch.float32, only=None):
    from sgv3d_amd import conv_grad
    n = 0
    for pad, dil, H, W, x, w, dy, y_ref, dx_ref, dw_ref in _grad_cases(k, stride, cin, cout):
        if only is not None and not only(pad, dil, H, W):
            continue
        xg, dyg = x.to(dtype).cuda().requires_grad_(True), dy.to(dtype).cuda()
        need_dw = dtype == torch.float32 or conv_grad._bf16_wgrad_ok(xg, dyg, cin, cout, 0, 0)      # (bf16 tensors: no other kernel reads them)
        wg = w.cuda().requires_grad_(need_dw)
        y = conv_grad.conv2d(xg, wg, None, stride, pad, dil)
        y.backward(dyg)
        tag = (k, stride, pad, dil, H, W, cin, cout)
        assert y.dtype == dtype and xg.grad.dtype == dtype
        assert torch.equal(y.detach().cpu(), y_ref.float().to(dtype)), ("y",) + tag
        assert torch.equal(xg.grad.cpu(), dx_ref.float().to(dtype)), ("dx",) + tag
        if need_dw:
            assert wg.grad.dtype == torch.float32 and torch.equal(wg.grad.cpu().double(), dw_ref), ("dw",) + tag
        n += 1
    return n


@pytest.mark.parametrize("k,stride", KS)
def test_conv2d_grad_fixed_rule(ops, k, stride):
    n = sum(_run_grad(k, stride, cin, cout) for cin, cout in ((8, 12), (32, 40)))
    print(f"[conv-geometry] grad k{k} s{stride} rule: {n} cases exact")


@pytest.mark.parametrize("tile", (1, 4, 44))
@pytest.mark.parametrize("k,stride", KS)
def test_conv2d_grad_forced_tile(ops, monkeypatch, k, stride, tile):
    """Every PackedConv that conv_grad builds (forward, rotated layer, phases, patchify) runs on one tile.  The five-per-CU tile (44)
    reads channel-chunk-major weights: it takes the cases whose layers -- the forward one and those ``dgrad_forms`` lists -- all read a
    multiple of 32 channels, so it has a channel pair of its own (the issue's pairs leave it none)."""
    from sgv3d_amd import conv_grad
    from sgv3d_amd.hip_ops import PackedConv
    monkeypatch.setattr(conv_grad, "PackedConv", functools.partial(PackedConv, tile=tile))
    n = 0
    for cin, cout in ((8, 12), (32, 40)) + (((32, 32),) if tile == 44 else ()):
        only = None
        if tile == 44:
            only = lambda pad, dil, H, W: cin % 32 == 0 and all(f.cin % 32 == 0 for f in G.dgrad_forms(k, stride, pad, dil, H, W, cin, cout))
        n += _run_grad(k, stride, cin, cout, only=only)
    assert n > 0
    print(f"[conv-geometry] grad k{k} s{stride} tile {tile}: {n} cases exact")


@pytest.mark.parametrize("k,stride", KS)
def test_conv2d_grad_bf16_products(ops, monkeypatch, k, stride):
    _set_mode(monkeypatch, ops, "bf16")
    n = sum(_run_grad(k, stride, cin, cout) for cin, cout in ((8, 12), (32, 40)))
    print(f"[conv-geometry] grad k{k} s{stride} bf16 products: {n} cases exact")


@pytest.mark.parametrize("k,stride", KS)
def test_conv2d_grad_bf16_storage(ops, monkeypatch, k, stride):
    """bf16 x and dy: bf16 y and dx (the exact value rounded once), f32 dw where the bf16 weight-gradient kernel takes the layer."""
    _set_mode(monkeypatch, ops, "bf16")
    no_patchify = lambda pad, dil, H, W: not (k == stride and stride > 1 and pad == 0 and dil == 1)
    n = sum(_run_grad(k, stride, cin, cout, torch.bfloat16, no_patchify) for cin, cout in ((8, 16), (32, 40)))
    assert n > 0
    print(f"[conv-geometry] grad k{k} s{stride} bf16 storage: {n} cases exact")


def test_bf16_storage_refusals(ops, monkeypatch):
    """What the bf16-storage sweep leaves out is refused, not mishandled: patchify data gradients, thin weight gradients."""
    from sgv3d_amd import _lib, conv_grad
    _set_mode(monkeypatch, ops, "bf16")
    dy = torch.zeros(2, 3, 3, 16, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(AssertionError, match="no patchify"):
        conv_grad.conv2d_backward_data(dy, torch.zeros(16, 8, 2, 2, device="cuda"), (6, 6), 2, 0, 1)
    x = torch.zeros(2, 5, 5, 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.SGV3DError, match="at least 16 channels"):
        conv_grad.conv2d_backward_weight(x, dy, 3, 1, 0, 1)
