"""CPU: the tile lattice of the three-launch F(4x4) path (csrc/conv_wino4.hip: wino4_axis / wino4_axis_pixels, the functions the
transform kernels decode their rows and columns with) through its host entry point sgv3d_wino4_lattice_axis, against brute force for
every axis length 1..40 and dilation 1..20: the tile count is the smaller of the two forms, every pixel is produced by exactly one
(tile, slot), no separator or out-of-axis slot maps to a pixel, and the six inputs of a tile are the 3x3's neighbours (pixel -+ dil,
or zero outside the axis) of its four outputs."""
import ctypes

import pytest

from sgv3d_amd import _lib, hip_ops

NS, DILS = range(1, 41), range(1, 21)


def _axis(lib, n, dil):
    tiles, stacked = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.sgv3d_wino4_lattice_axis(n, dil, 0, 0, 0, ctypes.addressof(tiles), ctypes.addressof(stacked), None) == 0
    return tiles.value, stacked.value


def _pixels(lib, n, dil, tile, k0, count):
    buf = (ctypes.c_int * 6)(*([-7] * 6))
    assert lib.sgv3d_wino4_lattice_axis(n, dil, tile, k0, count, None, None, ctypes.addressof(buf)) == 0, lib.sgv3d_last_error()
    assert list(buf[count:]) == [-7] * (6 - count)
    return list(buf[:count])


def test_tile_count_is_the_smaller_form():
    lib = _lib.load()
    for n in NS:
        for dil in DILS:
            split = dil * -(-(-(-n // dil)) // 4)
            stacked = -(-(n + dil - 1) // 4)
            tiles, is_stacked = _axis(lib, n, dil)
            assert tiles == min(split, stacked), (n, dil)
            assert is_stacked == int(stacked < split), (n, dil)                 # split on a tie
            assert hip_ops.wino4_axis_tiles(n, dil) == tiles, (n, dil)
    for n in NS:                                                                # dil 1: the plain map, tile t = pixels 4 t .. 4 t + 3
        tiles, is_stacked = _axis(lib, n, 1)
        assert (tiles, is_stacked) == (-(-n // 4), 0)
        for t in range(tiles):
            assert _pixels(lib, n, 1, t, -1, 6) == [c if 0 <= c < n else -1 for c in range(4 * t - 1, 4 * t + 5)]


def test_every_pixel_once_and_neighbours_of_its_own_phase():
    lib = _lib.load()
    seen_stacked = seen_split = empty_phase = 0
    for n in NS:
        for dil in DILS:
            tiles, is_stacked = _axis(lib, n, dil)
            seen_stacked += is_stacked
            seen_split += 1 - is_stacked
            empty_phase += int(dil > n)
            owner = {}
            for t in range(tiles):
                out = _pixels(lib, n, dil, t, 0, 4)
                inp = _pixels(lib, n, dil, t, -1, 6)
                assert inp[1:5] == out, (n, dil, t)
                for k, c in enumerate(out):
                    if c < 0:
                        continue
                    assert 0 <= c < n and c not in owner, (n, dil, t, k, c)
                    owner[c] = (t, k)
                    # the taps of the 3x3 at this output: the pixel dil to either side, or the zero padding outside the axis
                    assert inp[k] == (c - dil if c - dil >= 0 else -1), (n, dil, t, k, inp)
                    assert inp[k + 2] == (c + dil if c + dil < n else -1), (n, dil, t, k, inp)
                for c in (inp[0], inp[5]):
                    assert -1 <= c < n
            assert sorted(owner) == list(range(n)), (n, dil)                   # every pixel exactly once, nothing else
    assert seen_stacked > 100 and seen_split > 100 and empty_phase > 100


def test_the_counts_of_the_aspp_branches():
    """54x96 (cfg-2) and 68x120 (cfg-3): dilation 6 and 12 stack the rows only, dilation 18 the columns only at 54x96."""
    lib = _lib.load()
    got = {d: (_axis(lib, 54, d), _axis(lib, 96, d)) for d in (6, 12, 18)}
    assert got == {6: ((15, 1), (24, 0)), 12: ((17, 1), (24, 0)), 18: ((18, 0), (29, 1))}
    assert [hip_ops.wino4_tiles(1, 54, 96, d) for d in (1, 6, 12, 18)] == [336, 360, 408, 522]
    assert [hip_ops.wino4_tiles(4, 68, 120, d) for d in (6, 12, 18)] == [4 * a * b for a, b in ((18, 30), (20, 33), (18, 35))]


def test_refusals():
    lib = _lib.load()
    buf = (ctypes.c_int * 6)()
    for args in ((0, 1, 0, 0, 1), (5, 0, 0, 0, 1), (5, 2, 99, 0, 4), (5, 2, -1, 0, 4), (5, 2, 0, 1, 4), (5, 2, 0, 0, 7), (5, 2, 0, -1, 0)):
        assert lib.sgv3d_wino4_lattice_axis(*args, None, None, ctypes.addressof(buf)) != 0, args
