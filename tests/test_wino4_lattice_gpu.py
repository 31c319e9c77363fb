"""The tile lattice of the three-launch F(4x4) path on dilated layers (csrc/conv_wino4.hip: the phases of an axis stacked on one
line with a zero separator where that needs fewer tiles, tests/test_wino4_lattice_cpu.py for the index map itself), the global
average pool with 16-byte loads (csrc/misc_layers.hip, csrc/avgpool.hpp), on the guard-banded buffers of tests/wino_edges.py.

Exact data.  x in {-1, 0, 1}; every kept 3x3 kernel has ONE tap, +-576 = +-24^2, the others zero.  G g G^T of such a kernel is, entry
by entry, ONE product of a multiple of 24 with 1/4, 1/6, 1/12 or 1/24 per stage -- correctly rounded to the integer it stands for,
however the compiler contracts the packer's sums (with several taps a fused multiply-add keeps the 2^-25 error of 1/6 unrounded).  So U
is integer (|U| <= 144), V = B^T d B is integer (|V| <= 100), the f32x3 split of either is exact, every partial sum of a position
GEMM is an integer below 128 * 100 * 144 < 2^24 and A^T M A stays integer; scale 1 / 64 and integer shifts and residuals keep the
epilogue exact.  A tile's result then does not depend on what else its 6x6 inputs hold: any tiling gives the float64 convolution
bit for bit, and the bar is equality."""
import functools

import pytest
import torch

import wino_edges as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = 128
F4_IDS = [9, 10, 15, 46, 47]
DILS = (1, 2, 3, 6, 12, 18)
MAPS = [(1, 7, 19), (1, 19, 7), E.BIG]


@functools.lru_cache(maxsize=None)
def params():
    g = E._gen(71, 0)
    keep = torch.rand(C, C, generator=g) < 0.25
    tap = torch.randint(0, 9, (C, C), generator=g)
    sign = torch.randint(0, 2, (C, C), generator=g).float() * 2 - 1
    w = torch.zeros(C, C, 9)
    w.scatter_(2, tap[..., None], (sign * keep * 576.0)[..., None])
    return dict(w=w.view(C, C, 3, 3), sc=torch.full((C,), 1.0 / 64.0), sh=torch.randint(-2, 3, (C,), generator=g).float())


@functools.lru_cache(maxsize=None)
def case(geom, dil, residual=False):
    """(x, residual or None, float64 reference of conv + BN [+ residual] + ReLU): computed once per (map, dilation)."""
    p = params()
    B, H, W = geom
    g = E._gen(72, B, H, W, dil)
    x = torch.randint(-1, 2, (B, H, W, C), generator=g).float()
    res = torch.randint(-3, 4, (B, H, W, C), generator=g).float() if residual else None
    ref = E.epilogue64(E.conv64(x, p["w"], pad=dil, dil=dil), p["sc"], p["sh"], res, relu=True)
    assert E.exact_in_f32(ref)
    return x, res, ref


@pytest.fixture(scope="module")
def conv():
    from sgv3d_amd.hip_ops import PackedConv
    cache = {}

    def get(dil, affine=True):
        if (dil, affine) not in cache:
            p = params()
            kw = dict(scale=p["sc"].to(DEV), shift=p["sh"].to(DEV), relu=True) if affine else {}
            cache[dil, affine] = PackedConv(p["w"].to(DEV), pad=dil, dil=dil, **kw)
            assert cache[dil, affine].wino4_ok()
        return cache[dil, affine]
    return get


def _run(conv, geom, x, tile, residual=None):
    """x in channels [8, 8 + C) of a guarded [.., C + 16] map, y into channels [4, 4 + C) of a guarded [.., C + 12] buffer, the
    residual in channels [0, C) of a guarded [.., C + 8] map."""
    B, H, W = geom
    xg = E.guarded_input(x, C + 16, 8, DEV)
    rg = None if residual is None else E.guarded_input(residual, C + 8, 0, DEV)

    def run():
        out = E.GuardedOutput((B, H, W, C + 12), (W + 1) * (C + 12), DEV)
        conv(xg, out.view, x_coff=8, y_coff=4, residual=rg, tile=tile, split_k=1)
        return out
    return run


def _check(run, ref, window=(4, C)):
    out = run()
    got, intact = out.result(window)
    assert not bool(torch.isnan(got).any()), "a read outside the map (or outside the channel window) reached an output"
    assert intact, "a store outside the output window"
    assert tuple(got.shape) == tuple(ref.shape)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert torch.equal(out.flat, run().flat), "two runs differ"


def _x3():
    from sgv3d_amd.conv_tiles import family
    return list(family("wino4_x3"))


def test_the_maps_reach_every_combination_of_stacked_axes():
    from sgv3d_amd.hip_ops import wino4_axis_tiles
    stacked = lambda n, d: wino4_axis_tiles(n, d) < d * -(-(-(-n // d)) // 4)
    seen = {(stacked(H, d), stacked(W, d)) for _, H, W in MAPS for d in DILS}
    assert seen == {(False, False), (True, False), (False, True), (True, True)}
    assert all(not stacked(n, 1) for n in range(1, 60))


@pytest.mark.parametrize("geom", MAPS, ids=E.gid)
@pytest.mark.parametrize("dil", DILS)
@pytest.mark.parametrize("tile", ["f32", "x3"])
def test_lattice_exact_on_every_stacking(conv, tile, dil, geom):
    """The f32 path (TILE_WINO4) and the f32x3 path (64 x 128) at dilation 1, 2, 3, 6, 12, 18 on 7x19, 19x7 and 2x35x49 (both axes
    stacked, rows only, columns only, neither; batch 2), with a residual and ReLU, input and output in channel windows."""
    t = 9 if tile == "f32" else _x3()[1]
    x, res, ref = case(geom, dil, residual=True)
    _check(_run(conv(dil), geom, x, t, residual=res), ref)


@pytest.mark.parametrize("tile", F4_IDS + list(range(50, 60)))
def test_every_tile_id_on_a_stacked_map(conv, tile):
    """Every F(4x4) id -- the rows per position pad to 32, 48, 64, 96, 112 or 128 -- at dilation 6 on 19x7 and 7x19."""
    assert sorted(t for t in F4_IDS + _x3()) == sorted(F4_IDS + list(range(50, 60)))
    for geom in MAPS[:2]:
        x, _, ref = case(geom, 6)
        _check(_run(conv(6), geom, x, tile), ref)


@pytest.mark.parametrize("geom,dil", [((1, 1, 33), 2), ((1, 1, 33), 12), ((1, 3, 9), 6), ((1, 1, 1), 3), ((1, 2, 2), 18), ((1, 5, 40), 7)],
                         ids=lambda v: E.gid(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("tile", ["f32", "x3"])
def test_empty_phases_and_one_row_maps(conv, tile, geom, dil):
    """dil > H (phases without a pixel: a separator alone), a one-row and a one-pixel map."""
    t = 9 if tile == "f32" else _x3()[0]
    x, _, ref = case(geom, dil)
    _check(_run(conv(dil), geom, x, t), ref)


@pytest.mark.parametrize("tile", ["f32", "x3"])
@pytest.mark.parametrize("dil", [1, 6, 12])
def test_group_planes_on_the_lattice(conv, tile, dil):
    """GROUP_PLANES output ([cout / 64][B][H][W][64]) of a stacked layer, into a guarded buffer."""
    t = 9 if tile == "f32" else _x3()[1]
    geom = (2, 7, 19)
    B, H, W = geom
    x, _, ref = case(geom, dil)
    xg = E.guarded_input(x, C + 16, 8, DEV)

    def run():
        out = E.GuardedOutput((C // 64, B, H, W, 64), (W + 1) * 64, DEV)
        conv(dil)(xg, out.view, x_coff=8, group_planes=64, tile=t, split_k=1)
        return out
    out = run()
    got, intact = out.result()
    assert intact and torch.equal(got.permute(1, 2, 3, 0, 4).reshape(B, H, W, C), ref)
    assert torch.equal(out.flat, run().flat)


def test_dilation_one_keeps_its_bits(conv):
    """A dil = 1 layer is the parent's map tile for tile (the lattice of dil 1 IS ceil(n / 4) tiles from pixel 0): on the exact
    data its result is the float64 convolution bit for bit, on every F(4x4) id, on the sweep's ragged maps -- and the full-density
    data of tests/wino_edges.py (not exact: the packer rounds 1 / 6) stays inside that sweep's 2e-6 of S."""
    for geom in [(1, 1, 1), (1, 4, 4), (1, 5, 9), (1, 17, 17), E.BIG]:
        x, _, ref = case(geom, 1)
        for t in (9, 47, _x3()[0], _x3()[4]):
            _check(_run(conv(1), geom, x, t), ref)
    from sgv3d_amd.hip_ops import PackedConv
    p = E.wino4_params()
    full = PackedConv(p["w"].to(DEV), pad=1, scale=p["sc"].to(DEV), shift=p["sh"].to(DEV), relu=True)
    x, ref, S = E.wino4_case(E.BIG, 1)
    for t in (9, _x3()[1]):
        got, intact = _run(full, E.BIG, x, t)().result((4, C))
        assert intact and float((got - ref).abs().max()) <= 2e-6 * S


@pytest.mark.parametrize("dil,geom", [(6, (1, 13, 22)), (12, (2, 35, 49)), (18, (1, 20, 41))], ids=lambda v: E.gid(v) if isinstance(v, tuple) else str(v))
def test_random_floats_within_the_f4x4_bar(dil, geom):
    """Random float data against float64: the bar of tests/test_conv_wino_gpu.py for these kernels, 1e-4 of the output scale."""
    from sgv3d_amd.hip_ops import PackedConv
    B, H, W = geom
    g = E._gen(73, dil)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    res = torch.randn(B, H, W, C, generator=g)
    pc = PackedConv(w.to(DEV), pad=dil, dil=dil, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    ref = E.epilogue64(E.conv64(x, w, pad=dil, dil=dil), sc, sh, res, relu=True)
    bar = 1e-4 * max(1.0, float(ref.abs().max()))
    for t in (9, _x3()[1]):
        got, intact = _run(pc, geom, x, t, residual=res)().result((4, C))
        err = float((got - ref).abs().max())
        print(f"dil {dil} {E.gid(geom)} tile {t}: max err {err:.2e}, bar {bar:.2e}")
        assert intact and not bool(torch.isnan(got).any()) and err < bar


# ------------------------------------------------------------------------------------------------- global average pool
@pytest.mark.parametrize("P", [1, 5, 5184])
@pytest.mark.parametrize("Cn", [4, 60, 512])
def test_global_avgpool_quads(Cn, P):
    """sgv3d_global_avgpool with 16-byte loads against a float64 mean, the channels a slice of a wider map (ld = C + 12) and an
    unpadded one; batch 2.  Bound: a sum of n numbers added in ANY order is within (n - 1) eps sum |x_i| of the exact one (every
    partial sum is below sum |x|), here n = P, and the division rounds once more: P eps mean |x| per output -- summation order
    is the only thing the kernel may differ in.  Exact on small integers, bitwise repeatable, nothing outside [B, C] written."""
    from sgv3d_amd import _lib
    lib, B, eps = _lib.load(), 2, 2.0 ** -24
    for ld in (Cn, Cn + 12):
        g = E._gen(74, Cn, P, ld)
        for exact in (True, False):
            x = torch.randint(-3, 4, (B, P, ld), generator=g).float() if exact else torch.randn(B, P, ld, generator=g)
            xd = x.to(DEV)
            nbytes = lib.sgv3d_global_avgpool_workspace_bytes(B, Cn)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            outs = []
            for _ in range(2):
                out = E.GuardedOutput((B, Cn), 64, DEV)
                _lib.check(lib.sgv3d_global_avgpool(B, P, Cn, ld, xd.data_ptr(), out.view.data_ptr(), ws.data_ptr(), nbytes,
                                                    _lib.stream_handle()), "global_avgpool")
                outs.append(out)
            got, intact = outs[0].result()
            assert intact and torch.equal(outs[0].flat, outs[1].flat)
            want = x[..., :Cn].double().mean(1)
            if exact and P & (P - 1) == 0:
                assert torch.equal(got, want)
            else:
                bound = P * eps * x[..., :Cn].double().abs().mean(1) + 1e-30
                assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
