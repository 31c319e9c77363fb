"""CPU: what tests/test_wino_edges_gpu.py rests on -- the geometry list covers every tile and block remainder, the exact-data
references are float32 numbers (so that bit equality means something), the F(4x4) intermediates of that data stay exact in
float32, and the fused heads' block decomposition with the ring fix-up's index map, restated in tests/wino_edges.py, gives
the float64 definition -- and no longer does on the geometries named here once the zeroing of hidden pixels outside the image
or one ring index is changed (the sharpness of the GPU sweep, shown without running a broken kernel)."""
import pytest
import torch

import wino_edges as E


def test_geometries_cover_every_tile_and_block_remainder():
    """In the style of test_batchnorm_shapes_cover_the_kernel_paths: the property the sweep is there for."""
    assert sorted(h for _, h, _ in E.SWEEP) == sorted(w for _, _, w in E.SWEEP) == list(range(1, 34))
    for dim in (1, 2):                                               # H, W
        for lo, hi in ((1, 16), (17, 33)):                           # single-block maps, two- and three-block maps
            sizes = [g[dim] for g in E.SWEEP if lo <= g[dim] <= hi]
            assert {s % 4 for s in sizes} == set(range(4)) and {s % 16 for s in sizes} == set(range(16)), (dim, lo)
        assert {1, 2, 3} <= {g[dim] for g in E.SWEEP}                # smaller than one tile
    assert all(g in E.GEOMS for g in E.NAMED + [E.BIG]) and len(E.GEOMS) == len(set(E.GEOMS)) == 38
    assert all(b == 1 for b, _, _ in E.GEOMS[:-1])
    # one block, ragged on both sides at once; an interior block with all eight neighbours, ragged on both edges, batch 2
    assert any(h < 16 and w < 16 and h % 4 and w % 4 for _, h, w in E.GEOMS)
    B, H, W = E.BIG
    assert B == 2 and -(-H // 16) >= 3 and -(-W // 16) >= 3 and H % 16 and W % 16 and H % 4 and W % 4
    # the dilated pair: sub-grids of 4 and 3 rows and of 10 and 9 columns, and the same swapped
    assert [sorted({-(-(n - p) // 2) for p in (0, 1)}) for n in E.DILATED[0][1:]] == [[3, 4], [9, 10]]
    assert E.DILATED[1] == (1, E.DILATED[0][2], E.DILATED[0][1])


@pytest.mark.parametrize("name", ["head_f4", "head_f2", "f4res_64to64", "f4res_64to128", "f4res_128to64", "wino2"])
def test_exact_references_are_float32_numbers(name):
    ref = {"head_f4": lambda: E.head_f4_case(E.BIG)[1], "head_f2": lambda: E.head_f2_case(E.BIG)[1],
           "wino2": lambda: E.wino2_case(E.BIG)[1]}.get(name, lambda: E.f4res_case(name[6:], E.BIG)[2])()
    assert ref.dtype == torch.float64 and E.exact_in_f32(ref)
    assert float(ref.abs().max()) > 8                                # not a degenerate case
    if name == "head_f2":                                            # hidden maps in quarters: the outputs as well
        assert bool((ref * 4 == (ref * 4).round()).all()) and float(ref.abs().max()) * 4 < 2.0 ** 24
        assert bool((ref != ref.round()).any())
    if name.startswith("head"):
        p = E.head_f4_params() if name == "head_f4" else E.head_f2_params()
        x = (E.head_f4_case if name == "head_f4" else E.head_f2_case)(E.BIG)[0]
        hid = E.hidden64(x, p)                                       # every partial sum of the final convolution is below this
        assert float(hid.max()) * (4 if name == "head_f2" else 1) * 64 * 9 * 2 < 2.0 ** 24 and float((hid > 0).double().mean()) > 0.2


@pytest.mark.parametrize("name", ["head_f4", "f4res_64to128", "f4res_128to64"])
def test_f4_intermediates_of_the_exact_data_stay_exact(name):
    """U = G g G^T is integer for taps that are multiples of 576, V = B^T d B is integer, and every partial sum of the position
    GEMMs and of A^T M A is an integer below 2^24: the F(4x4) kernels reproduce the float64 definition bit for bit, in any
    summation order.  (The restatement itself is checked against the convolution.)"""
    if name == "head_f4":
        x, w = E.head_f4_case(E.BIG)[0], E.head_f4_params()["w1"]
    else:
        x, w = E.f4res_case(name[6:], E.BIG)[0], E.f4res_params(name[6:])["w"]
    y, u_integer, acc_bound, y_bound = E.f4_intermediates(x, w)
    assert torch.equal(y, E.conv64(x, w))
    assert u_integer and acc_bound < 2.0 ** 24 and y_bound < 2.0 ** 24, (acc_bound, y_bound)


BLOCK_GEOMS = [(1, 1, 1), (1, 16, 16), (1, 13, 22), (1, 17, 17), (1, 33, 30), E.BIG]


@pytest.fixture(scope="module")
def by_blocks():
    """geometry -> (float64 reference, the restated block decomposition), computed once."""
    cache = {}

    def get(geom):
        if geom not in cache:
            x, ref = E.head_f4_case(geom)
            cache[geom] = (x, ref, E.head_by_blocks(x, E.head_f4_params()))
        return cache[geom]
    return get


@pytest.mark.parametrize("geom", BLOCK_GEOMS, ids=E.gid)
def test_heads_by_blocks_restatement_is_the_definition(by_blocks, geom):
    assert geom in E.GEOMS
    _, ref, got = by_blocks(geom)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("geom", BLOCK_GEOMS, ids=E.gid)
def test_unzeroed_hidden_pixels_outside_the_image_cannot_pass(by_blocks, geom):
    """head_wino4_kernel's `if (!full) hd = in ? hd : 0` (conv_wino_head_kernel's `in ? ... : 0.f`): without it a hidden pixel
    just outside the image holds ReLU(BN(first layer of the zero-padded input)) and leaks into the border outputs.  Every map
    with a ragged block reaches that line -- the one-pixel map included -- and the exact comparison then fails; 16x16 cannot
    see it."""
    x, ref, _ = by_blocks(geom)
    leaky = E.head_by_blocks(x, E.head_f4_params(), zero_outside=False)
    ragged = geom[1] % 16 != 0 or geom[2] % 16 != 0
    assert torch.equal(leaky, ref) == (not ragged)
    if ragged:                                   # wrong by whole products, on the border the ragged side touches
        bad = (leaky != ref).nonzero()
        assert float((leaky - ref).abs().max()) >= 1.0
        assert all(int(y) == geom[1] - 1 or int(xx) == geom[2] - 1 for _, _, y, xx in bad)


def _sources_with(slot_from, slot_to):
    return lambda py, px: [(dy, dx, slot_to if s == slot_from else s) for dy, dx, s in E.ring_sources(py, px)]


@pytest.mark.parametrize("geom", BLOCK_GEOMS, ids=E.gid)
@pytest.mark.parametrize("slot_from,slot_to,needs", [(18, 19, "diagonal"), (0, 1, "diagonal"), (35, 34, "diagonal"), (17, 16, "diagonal"),
                                                     (20, 21, "below"), (55, 56, "right")])
def test_one_wrong_ring_index_cannot_pass(by_blocks, geom, slot_from, slot_to, needs):
    """One slot of head_ring_fixup_kernel's index map moved by one: the four corner slots (read from the diagonal
    neighbours) need two blocks each way -- 17x17 is the smallest such map --, a slot of a block's bottom row is read by the
    block below it, a slot of its right column by the block to its right.  Where the geometry reaches the slot the exact
    comparison fails."""
    x, ref, _ = by_blocks(geom)
    nby, nbx = -(-geom[1] // 16), -(-geom[2] // 16)
    reached = {"diagonal": nby > 1 and nbx > 1, "below": nby > 1 and geom[2] > 1, "right": nbx > 1 and geom[1] > 3}[needs]
    got = E.head_by_blocks(x, E.head_f4_params(), sources=_sources_with(slot_from, slot_to))
    assert torch.equal(got, ref) == (not reached)
