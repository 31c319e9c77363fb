"""CPU: what tests/test_head_bf16_edges_gpu.py rests on.  The geometry list covers every remainder of the bf16 head's 16 x 16 tile
and of its 4-pixel store group, in both dimensions and at both parities of the width; the exact data of tests/head_bf16_edges.py
keeps every partial sum of both layers a float32 number (so that bit equality with the float64 contract means something) while
the bf16 roundings of x, w1 and the hidden map change a stated share of the values, exact ties among them; the kernel's tile
decomposition, restated on the CPU, gives the contract -- and no longer does once the hidden map is truncated, rounded with ties
away from zero or left unrounded, x is truncated, w1 is left unrounded, or the hidden pixels outside the image are not zeroed
(the sharpness of the GPU sweep, shown without running a broken kernel)."""
import pytest
import torch

import head_bf16_edges as E
import wino_edges


def test_geometries_cover_every_tile_and_store_remainder():
    """wino_edges.SWEEP's property, restated for this kernel: tile 16, store groups of 4."""
    assert E.GEOMS is wino_edges.GEOMS and len(E.GEOMS) == 38
    for dim in (1, 2):                                               # H, W
        for lo, hi in ((1, 16), (17, 33)):                           # one tile; two and three tiles
            sizes = [g[dim] for g in E.GEOMS if lo <= g[dim] <= hi]
            assert {s % E.TILE for s in sizes} == set(range(E.TILE)) and {s % E.STORE for s in sizes} == set(range(E.STORE)), (dim, lo)
        assert {1, 2, 3} <= {g[dim] for g in E.GEOMS}                # narrower than one store group
    # the 16-byte store path needs gx + 3 < W and an aligned address: (row * W) % 4 takes every value when W is odd, two when
    # W = 2 (mod 4); the start of plane k of image b is (b * total + k) * H * W floats: with total = 10 and H * W odd, the second
    # image's planes start at the other alignments
    assert {w % 2 for _, _, w in E.GEOMS} == {0, 1}
    B, H, W = E.BIG
    assert B == 2 and (H * W) % 2 == 1 and sum(E.COUNTS) % 2 == 0 and len({(k * H * W) % 4 for k in range(2 * sum(E.COUNTS))}) == 4
    assert -(-H // E.TILE) >= 3 and -(-W // E.TILE) >= 3 and H % E.TILE and W % E.TILE          # an interior tile, ragged both ways
    assert sorted(E.COUNTS) == [1, 2, 3, 4]
    assert all(g in E.GEOMS for g in E.BRANCH_GEOMS + [t for t in E.TILE_GEOMS if t != (1, 13, 22)])
    assert all(max(h, w) > E.TILE for _, h, w in E.BRANCH_GEOMS)                                # they cross a tile seam
    assert all(max(E.cycling_counts(n)) <= 4 for n in E.BRANCH_COUNTS) and set(E.cycling_counts(48)) == {1, 2, 3, 4}
    for ld, coff in E.F32_WINDOWS:
        assert ld % 4 == 0 and coff % 4 == 0 and coff + 64 <= ld
    for ld, coff in E.BF16_WINDOWS:
        assert ld % 8 == 0 and coff % 8 == 0 and coff + 64 <= ld


def test_round_bf16_modes():
    """The bit arithmetic of round_bf16: 'rne' is torch's conversion; the tie 1 + 2^-8 goes to 1 (even), 1 + 3 * 2^-8 to
    1 + 2^-6 (even); 'away' and 'trunc' do what they say, for both signs."""
    t = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * torch.tensor([1e-3, 1.0, 300.0, 1e5]).repeat(1024)
    assert torch.equal(E.round_bf16(t), t.bfloat16().double())
    v = torch.tensor([E.TIE_TAP, 1 + 3 * 2.0 ** -8, -E.TIE_TAP, 257 / 16.0, 1 + 2.0 ** -7, 1 + 2.0 ** -9 + 2.0 ** -8])
    assert E.round_bf16(v).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 16.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7]
    assert E.round_bf16(v, "away").tolist() == [1 + 2.0 ** -7, 1 + 2.0 ** -6, -(1 + 2.0 ** -7), 16.125, 1 + 2.0 ** -7, 1 + 2.0 ** -7]
    assert E.round_bf16(v, "trunc").tolist() == [1.0, 1 + 2.0 ** -7, -1.0, 16.0, 1 + 2.0 ** -7, 1.0]
    assert torch.equal(E.round_bf16(v, "none"), v.double())
    assert E.changed_and_ties(v) == (5 / 6, 4 / 6) and E.changed_and_ties(torch.tensor([1 + 2.0 ** -9, 1.0])) == (0.5, 0.0)


def _cases():
    return [(g, E.COUNTS) for g in E.GEOMS] + [(g, E.cycling_counts(n)) for g in E.BRANCH_GEOMS for n in E.BRANCH_COUNTS] \
        + [(g, (2, 0, 4, 1)) for g in E.BRANCH_GEOMS]


@pytest.mark.parametrize("geom,counts", _cases(), ids=[f"{E.gid(g)}-w{'.'.join(map(str, c)) if len(c) < 5 else len(c)}" for g, c in _cases()])
def test_exact_data_stays_exact_and_roundings_bite(geom, counts):
    """For every (map, branch structure) the GPU tests run: the reference is a float32 number everywhere; x and the hidden map
    lie on their grids; the a-priori bounds on every partial sum, in units of the grid, are below 2^24 -- layer 1 by
    conv(|x|, |w1|), the folded BN by |conv| * scale + |shift|, layer 2 by conv(hidden, |w2|) (no cancellation) plus the bias --,
    so the fp32 kernel reproduces the float64 contract bit for bit in any summation order.  The cruder layer-2 bound
    576 * max hidden * max |w2| is 16.2 M units at 2x35x49 (below 2^24) and above 2^24 for 48 branches; the one asserted is the
    sharper and equally valid one.  And the roundings change values: a fifth of x (nearly all of them ties), half of the
    nonzero w1 taps (all ties), three tenths of the positive hidden values (a tenth ties)."""
    x, p = E.head_x(geom), E.params(counts)
    ref = E.head_case(geom, counts)[1]
    assert ref.dtype == torch.float64 and E.exact_in_f32(ref) and tuple(ref.shape) == (geom[0], sum(counts), geom[1], geom[2])
    s = E.exactness(x, p)
    print(E.gid(geom), len(counts), s)
    assert s["x_on_grid"] and s["w1_rounded_is_ternary"] and s["hid_on_grid"]
    assert max(s["l1_bound"], s["bn_bound"], s["l2_bound"], s["out_bound"]) < 2.0 ** 24
    assert float(x.abs().max()) <= E.X_KMAX * E.X_UNIT
    assert s["w1_changed"][0] >= 0.4 and s["w1_changed"][1] == s["w1_changed"][0]
    assert s["hid_positive"] >= 0.2
    n = x.numel()
    if n >= 64 * 16:                    # shares of a random sample: asserted where the sample is large enough to have them
        assert s["x_changed"][0] >= 0.2 and s["x_changed"][1] >= 0.2
        assert s["hid_changed"][0] >= 0.3 and s["hid_changed"][1] >= 0.1
    else:                               # on the smallest maps: some of each at least
        assert s["x_changed"][1] > 0 and s["hid_changed"][1] > 0


def test_big_map_figures():
    """The figures quoted in head_bf16_edges.py for 2x35x49: tens of thousands of exact ties in x, a hidden map that reaches
    beyond 512 (where a bf16 step is 4, 128 grid units), outputs that are not integers."""
    x, ref = E.head_case(E.BIG)
    s = E.exactness(x, E.params())
    assert s["x_changed"][1] * x.numel() > 20000
    assert 512 < s["hid_max"] < 1024 and s["l2_worst"] < 2.0 ** 24
    assert bool((ref != ref.round()).any()) and float(ref.abs().max()) > 1000


@pytest.fixture(scope="module")
def by_tiles():
    """geometry -> (x, the contract on the whole map); head_case computes it once."""
    return E.head_case


@pytest.mark.parametrize("geom", E.TILE_GEOMS, ids=E.gid)
def test_tile_restatement_is_the_contract(by_tiles, geom):
    x, ref = by_tiles(geom)
    assert torch.equal(E.head_by_tiles(x, E.params()), ref)


@pytest.mark.parametrize("geom", E.TILE_GEOMS, ids=E.gid)
@pytest.mark.parametrize("change", [dict(hid_round="trunc"), dict(hid_round="away"), dict(hid_round="none"), dict(x_round="trunc"),
                                    dict(w1_round="none")], ids=lambda c: "-".join(f"{k}-{v}" for k, v in c.items()))
def test_a_wrong_rounding_cannot_pass(by_tiles, geom, change):
    """The kernel's decomposition with one rounding changed -- the hidden map truncated (a shift instead of a conversion),
    rounded with ties away from zero, or left in fp32; x truncated; w1 left unrounded -- differs from the exact reference on
    every one of these maps, the one-pixel map included, in most outputs and by half a unit or more (16 grid steps): torch.equal
    sees it.  In units of max |reference| at 2x35x49: truncated hidden map 3.7e-3, ties away 1.3e-3, unrounded 1.6e-3, truncated
    x 3.4e-3, unrounded w1 3.7e-3 -- the order of the 2e-3 bar of test_fused_centerhead_bf16, which therefore cannot tell."""
    x, ref = by_tiles(geom)
    got = E.head_by_tiles(x, E.params(), **change)
    assert not torch.equal(got, ref)
    assert float((got - ref).abs().max()) >= 0.5 and float((got != ref).double().mean()) > 0.5
    if geom == E.BIG:
        assert 1e-3 < float((got - ref).abs().max()) / float(ref.abs().max()) < 5e-3


@pytest.mark.parametrize("geom", E.TILE_GEOMS, ids=E.gid)
def test_unzeroed_hidden_pixels_outside_the_image_cannot_pass(by_tiles, geom):
    """`pk.u = hin[mt] ? pk.u : 0`: without it a hidden pixel outside the image holds ReLU(shift) (its patch is all zeros, or
    what the image's last pixels give it) and leaks into the border outputs.  Unlike the fp32 heads, where only a ragged block
    reaches the mask, every tile here recomputes its one-pixel ring: EVERY map sees it, 16x16 included, on all four borders;
    the interior pixels do not."""
    x, ref = by_tiles(geom)
    leaky = E.head_by_tiles(x, E.params(), zero_outside=False)
    assert not torch.equal(leaky, ref)
    _, H, W = geom
    bad = (leaky != ref).nonzero()
    assert all(int(y) in (0, H - 1) or int(xx) in (0, W - 1) for _, _, y, xx in bad)
    rows, cols = {int(y) for _, _, y, _ in bad}, {int(xx) for _, _, _, xx in bad}
    assert {0, H - 1} <= rows and {0, W - 1} <= cols
    assert float((leaky - ref).abs().max()) >= 0.25                     # a whole shift (quarters) times a tap of +-1


def test_guarded_bf16_input_layout():
    x = E.round_bf16(E.head_x((1, 3, 5))).float()
    v = E.guarded_input_bf16(x, 96, 24, "cpu")
    assert v.dtype == torch.bfloat16 and tuple(v.shape) == (1, 3, 5, 96) and v.is_contiguous()
    assert torch.equal(v[..., 24:88].float(), x)
    assert bool(torch.isnan(v[..., :24].float()).all()) and bool(torch.isnan(v[..., 88:].float()).all())
    with pytest.raises(AssertionError):
        E.guarded_input_bf16(x, 68, 0, "cpu")
    with pytest.raises(AssertionError):
        E.guarded_input_bf16(E.head_x((1, 3, 5)), 64, 0, "cpu")          # not bf16 numbers: the entry takes rounded x


def test_zero_width_branch_reference():
    p = E.params((2, 0, 4, 1))
    q = E.without_branch(p, 1)
    assert q["counts"] == (2, 4, 1) and q["w1"].shape[0] == 192 and torch.equal(q["w1"][64:], p["w1"][128:]) and q["w2"] is p["w2"]
    x = E.head_x((1, 17, 17))
    assert torch.equal(E.head_ref(x, p), E.head_ref(x, q)) and torch.equal(E.head_by_tiles(x, p), E.head_ref(x, q))


@pytest.mark.parametrize("ob,rows,nb,ok", [([0, 2, 7, 8], 8, 3, False), ([0, 3, 2, 6], 6, 3, False), ([0, 2, 4, 5], 6, 3, False),
                                           ([1, 2, 4, 6], 6, 3, False), (list(range(50)), 49, 49, False), ([0, 2, 2, 6], 6, 3, True)])
def test_pack_centerhead_bf16_checks_the_table_on_the_host(monkeypatch, ob, rows, nb, ok):
    """The packer's refusals need no GPU: a branch of 5, a decreasing table, a wrong total, a table that does not start at 0 and
    49 branches raise ValueError before the library is even loaded; widths (2, 0, 4) pass the check (and reach the loader)."""
    from sgv3d_amd import _lib, hip_ops

    class Reached(Exception):
        pass

    def load():
        raise Reached()
    monkeypatch.setattr(_lib, "load", load)
    with pytest.raises(Reached if ok else ValueError):
        hip_ops.pack_centerhead_bf16(torch.zeros(nb * 64, 64, 3, 3), torch.zeros(rows, 3, 3, 64), torch.tensor(ob, dtype=torch.int32))
