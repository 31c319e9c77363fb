"""The index arithmetic of the Winograd kernels -- 4x4 tiles, 16x16 blocks, the one-pixel ring between blocks, zeroing of hidden
pixels outside the image, ragged stores -- at every tile and block remainder (tests/wino_edges.py: GEOMS), against F.conv2d in
float64.  Every input lies inside a larger NaN-filled allocation, in a channel window of a wider tensor whose other channels
are NaN, and every output inside a larger buffer of sentinels: a read outside the map that reaches an output shows up as NaN,
a stray store as a changed sentinel.  Each case also runs twice and compares the bits.  Exact data wherever the arithmetic allows
it, so that the bar is bit equality (tests/test_wino_edges_cpu.py: why it means something, and which geometry catches what)."""
import pytest
import torch

import wino_edges as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
F4_IDS = [9, 10, 15, 46, 47]          # hip_ops.TILE_WINO4, _WIDE, _NARROW, _OCC, _G48; the f32x3 ids come from WINO4_X3_TILES


def _finish(out, window, ref, rerun):
    """The checks every case ends with: no NaN, sentinels intact, a second run gives the same bits.  Returns the result."""
    got, intact = out.result(window)
    assert not bool(torch.isnan(got).any()), "a read outside the map (or outside the channel window) reached an output"
    assert intact, "a store outside the output window"
    assert tuple(got.shape) == tuple(ref.shape)
    again = rerun()
    assert torch.equal(out.flat, again.flat), "two runs differ"
    return got


# ---------------------------------------------------------------------------------------------- (a), (e): the fused heads
def _run_head(call, geom, x, ld=64 + 16):
    B, H, W = geom
    xg = E.guarded_input(x, ld, 0, DEV)                     # channels [0, 64) of an 80-channel map, the rest NaN

    def run():
        out = E.GuardedOutput((B, sum(E.COUNTS), H, W), W + 1, DEV)
        call(xg, out.view)
        return out
    return run


@pytest.fixture(scope="module")
def head_f4():
    from sgv3d_amd import hip_ops
    p = E.head_f4_params()
    ob = torch.tensor([0, E.COUNTS[0], sum(E.COUNTS)], dtype=torch.int32, device=DEV)
    args = (hip_ops.pack_centerhead_f4(p["w1"].to(DEV)), p["sc"].to(DEV), p["sh"].to(DEV),
            p["w2"].permute(0, 2, 3, 1).contiguous().to(DEV), p["b2"].to(DEV), ob, len(E.COUNTS))
    return lambda x, out: hip_ops.centerhead_branches_f4(x, *args, out=out)


@pytest.mark.parametrize("geom", E.GEOMS, ids=E.gid)
def test_fused_head_f4_exact_at_every_remainder(head_f4, geom):
    """(a) sgv3d_centerhead_branches_forward_f4 (head_wino4_kernel + head_ring_fixup_kernel), branches of 3 and 5 outputs, on
    the data of test_fused_centerhead_f4_exact_on_small_integers: bit equality with the float64 definition."""
    x, ref = E.head_f4_case(geom)
    run = _run_head(head_f4, geom, x)
    got = _finish(run(), None, ref, run)
    assert torch.equal(got, ref), float((got - ref).abs().max())


@pytest.fixture(scope="module")
def head_f2():
    from sgv3d_amd import hip_ops
    from sgv3d_amd.hip_ops import PackedConv
    p = E.head_f2_params()
    first = PackedConv(p["w1"].to(DEV), pad=1, scale=p["sc"].to(DEV), shift=p["sh"].to(DEV), relu=True)
    ob = torch.tensor([0, E.COUNTS[0], sum(E.COUNTS)], dtype=torch.int32, device=DEV)
    w2, b2 = p["w2"].permute(0, 2, 3, 1).contiguous().to(DEV), p["b2"].to(DEV)
    return lambda x, out: hip_ops.centerhead_branches(x, first, w2, b2, ob, len(E.COUNTS), out=out)


@pytest.mark.parametrize("geom", E.GEOMS, ids=E.gid)
def test_fused_head_f2_exact_at_every_remainder(head_f2, geom):
    """(e) sgv3d_centerhead_branches_forward (conv_wino_head_kernel + the same ring fix-up), cin 64, branches of 3 and 5
    outputs; integer x, w1, w2, b2 and shifts, scale 1 / 4: every intermediate is a multiple of 1 / 4 below 2^24 (the packer's
    G has halves only, the kernel adds and multiplies), so the bar is bit equality.  The branch of 5 is the case that found
    conv_wino_head_kernel writing only the first four outputs of a branch (its fifth plane kept whatever the buffer held); the
    kernel now runs the further outputs of a wide branch in passes of four."""
    x, ref = E.head_f2_case(geom)
    run = _run_head(head_f2, geom, x)
    got = _finish(run(), None, ref, run)
    assert torch.equal(got, ref), float((got - ref).abs().max())


# ----------------------------------------------------------------------------------------------------- NHWC convolutions
def _run_conv(conv, geom, x, cin, cout, tile, split_k=1, residual=None, finite=None):
    """``conv`` on x in channels [8, 8 + cin) of a guarded [.., cin + 16] map, into channels [4, 4 + cout) of a guarded
    [.., cout + 12] buffer; the residual, if any, in channels [0, cout) of a guarded [.., cout + 8] map."""
    B, H, W = geom
    xg = E.guarded_input(x, cin + 16, 8, DEV, finite=finite)
    rg = None if residual is None else E.guarded_input(residual, cout + 8, 0, DEV)

    def run():
        out = E.GuardedOutput((B, H, W, cout + 12), (W + 1) * (cout + 12), DEV)
        conv(xg, out.view, x_coff=8, y_coff=4, residual=rg, tile=tile, split_k=split_k)
        return out
    return run


def _packed(w, **kw):
    from sgv3d_amd.hip_ops import PackedConv
    return PackedConv(w.to(DEV), pad=kw.pop("pad", 1), **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()})


@pytest.fixture(scope="module")
def f4res():
    cache = {}

    def get(name):
        if name not in cache:
            p = E.f4res_params(name)
            cache[name] = _packed(p["w"], cin_pad=p["cin"], scale=p["sc"], shift=p["sh"], relu=True)
            assert cache[name].f4res_ok()
        return cache[name]
    return get


@pytest.mark.parametrize("name,geom", [("64to64", g) for g in E.GEOMS] + [(n, g) for n in ("64to128", "128to64") for g in E.NAMED + [E.BIG]],
                         ids=lambda v: v if isinstance(v, str) else E.gid(v))
def test_winograd4_resident_exact_at_every_remainder(f4res, name, geom):
    """(b) conv_f4res_kernel through PackedConv(tile=TILE_F4RES) with BN, an integer residual and ReLU: 64 -> 64 everywhere,
    64 -> 128 (two output tiles, one V) and 128 -> 64 (V rebuilt per chunk; 120 real input channels, the padded ones hold 7.0
    against zero weights) on the named maps and 2x35x49.  The head's exact construction: bit equality."""
    from sgv3d_amd.hip_ops import TILE_F4RES
    p = E.f4res_params(name)
    x, res, ref = E.f4res_case(name, geom)
    xin = torch.cat([x, torch.zeros(*x.shape[:3], p["cin"] - p["cin_real"])], -1)
    run = _run_conv(f4res(name), geom, xin, p["cin"], p["cout"], TILE_F4RES, residual=res,
                    finite=(p["cin_real"], 7.0) if p["cin"] > p["cin_real"] else None)
    got = _finish(run(), (4, p["cout"]), ref, run)
    assert torch.equal(got, ref), float((got - ref).abs().max())


@pytest.fixture(scope="module")
def wino4():
    cache = {}

    def get(dil):
        if dil not in cache:
            p = E.wino4_params()
            cache[dil] = _packed(p["w"], pad=dil, dil=dil, scale=p["sc"], shift=p["sh"], relu=True)
            assert cache[dil].wino4_ok()
        return cache[dil]
    return get


def _wino4_cases():
    from sgv3d_amd.conv_tiles import family, TILE_WINO4
    x3 = family("wino4_x3")
    cases = [(t, g, 1) for t in (TILE_WINO4, x3[1]) for g in E.GEOMS]
    cases += [(t, g, 1) for t in F4_IDS + list(x3) for g in E.SMALL3 if (t, g, 1) not in cases]
    cases += [(t, g, 2) for t in (TILE_WINO4, x3[1]) for g in E.DILATED]
    return cases


WORST = {}          # tile family -> worst error / S seen in this process (printed by the last test of the sweep)


@pytest.mark.parametrize("tile,geom,dil", _wino4_cases(), ids=lambda v: E.gid(v) if isinstance(v, tuple) else str(v))
def test_winograd_f4x4_geometry_at_every_remainder(wino4, tile, geom, dil):
    """(c) The three-launch F(4x4) (wino4_input_kernel / _x3 -> grouped position GEMM -> wino4_output_kernel), 128 -> 128 with
    BN and ReLU into a y_coff slice: TILE_WINO4 and one f32x3 id on every map, every F(4x4) id on 1x1, 7x19 and 2x35x49, and
    pad = dil = 2 on 7x19 and 19x7.  Data of test_winograd_f4x4_x3_keeps_every_partial_product (x in {-1, 0, 1}, w in
    {-1, 0, 1} x 576); the bar is 2e-6 of S = max conv(|x|, |w|), the scale of the products with no cancellation (that test's
    max |ref| means nothing on a one-pixel map).  A misplaced tile or pixel is wrong by a whole product, 1e-3 of S or more.
    This sweep guards GEOMETRY; the 24x40 test keeps guarding dropped partial products.
    Worst measured error / S on the MI355X over these 121 cases: 7.6e-8 for the f32 MFMA ids (9, 10, 15, 46, 47), 7.0e-8 for
    the f32x3 ids (50..59); 1.3e-8 on the one-pixel map."""
    from sgv3d_amd.conv_tiles import TILES
    x, ref, S = E.wino4_case(geom, dil)
    run = _run_conv(wino4(dil), geom, x, 128, 128, tile)
    got = _finish(run(), (4, 128), ref, run)
    err = float((got - ref).abs().max()) / S
    fam = TILES[tile].family
    WORST[fam] = max(WORST.get(fam, 0.0), err)
    print(f"F(4x4) tile {tile} ({fam}) {E.gid(geom)} dil {dil}: error / S = {err:.2e} (S = {S:.0f}); worst so far {WORST}")
    assert err <= 2e-6, (err, S)


@pytest.fixture(scope="module")
def wino2():
    conv = _packed(E.wino2_weight())
    assert conv.w_wino is not None
    return conv


@pytest.mark.parametrize("geom", E.GEOMS, ids=E.gid)
@pytest.mark.parametrize("tile,split_k", [(5, 1), (5, 2), (8, 1), (8, 2), (6, 1)])
def test_winograd_f2x2_exact_at_every_remainder(wino2, tile, split_k, geom):
    """(d) conv_wino_kernel (TILE_WINO = 5), conv_wino_half_kernel (TILE_WINO_HALF = 8), both at split_k 1 and 2, and
    conv_wino_resident_kernel (TILE_WINO_RES = 6), 32 -> 72 on integer data: bit equality, as
    test_winograd_bit_exact_on_integer_data asserts at 20x36."""
    x, ref = E.wino2_case(geom)
    run = _run_conv(wino2, geom, x, 32, 72, tile, split_k=split_k)
    got = _finish(run(), (4, 72), ref, run)
    assert torch.equal(got, ref), float((got - ref).abs().max())
