"""The host tile ids of the forward convolution: ONE record per id, pure data (no torch, no library, no environment).

A host tile id is what ``PackedConv`` is asked for (``tile=``), what the first-call measurement times, what ``tune/gfx950_*.json``
stores and what ``TUNE_DB`` / ``_tile_cache`` hold -- so the numbers never change.  It names an algorithm AND a workgroup shape; the C
ABI (include/sgv3d_hip.h) takes the algorithm as the entry point and the shape as ``desc.tile``.  Everything ``hip_ops`` knows about
an id comes from its record here; a new kernel variant is a new row.

    id, label     the id and the profile label (``hip_ops.TILE_NAMES``)
    family        igemm | wino | wino4 | wino4_x3 | f4res | pw_x3 | patch_bf16 | dw_bf16
    entry         the launcher / ABI entry-point family (``PackedConv._launch_<entry>``)
    abi           ``desc.tile`` as the entry point wants it (None: the entry point does not read it, the id is passed on)
    form          the packed weight form the kernel reads (``PackedConv._form``)
    bm, bn        the workgroup footprint in GEMM rows (pixels) x columns (channels) that grid estimates use
    spatial       None, or (tile height, tile width, input channels per k-step): the workgroup owns a 2-d patch of the map, so its
                  grid is batch x ceil(oh / th) x ceil(ow / tw) x ceil(n / bn) and its k-steps are cin / channels
    split         the split-K policy class (a key of SPLIT_POLICY), None = never split
    x3            products are f32-accurate sums of bf16 partial products ("f32x3")
    mfirst        the workgroups walk the channel tiles of one m-tile back to back (SGV3D_TILE_MFIRST)
    occ5          the five-workgroups-per-CU form of the 64x64 implicit-GEMM tile (SGV3D_TILE_OCC5)
    deep          direct-weight kernel: rows and fragments requested two k-chunks ahead
    only          'f32' / 'bf16': the mode the algorithm exists in (None: both)
    symbol        template of the MFMA kernel's symbol for the profile record; {chunk} / {pw} / {kmode} are filled per layer
    flops         the rule for the MFMA flops that kernel executes: 'direct' (m x n x k as padded), 'direct_k32' (k rounded up to
                  32), 'wino4' (36 positions x rows padded to bm x cin x cout); None: no record.  x3 tiles report six bf16 products each
"""
from collections import namedtuple

# --- desc.tile values: mirror of include/sgv3d_hip.h
SGV3D_TILE_128x128, SGV3D_TILE_128x64, SGV3D_TILE_64x128, SGV3D_TILE_64x64 = 1, 2, 3, 4
SGV3D_TILE_32x128, SGV3D_TILE_48x64 = 9, 10
SGV3D_TILE_MFIRST, SGV3D_TILE_OCC5, SGV3D_TILE_X3 = 16, 32, 64
SGV3D_WINOGRAD_RESIDENT, SGV3D_WINOGRAD_HALF = 6, 8
SGV3D_TILE_DW_64x256, SGV3D_TILE_DW_128x128, SGV3D_TILE_DW_256x64, SGV3D_TILE_DW_128x256, SGV3D_TILE_DW_256x128 = 31, 32, 33, 34, 35
SGV3D_TILE_DW_64x256_DEEP, SGV3D_TILE_DW_128x128_DEEP, SGV3D_TILE_DW_64x128, SGV3D_TILE_DW_64x128_DEEP = 36, 37, 38, 39

# --- host ids that code names
TILE_WINO = 5             # Winograd F(2x2,3x3) (sgv3d_conv2d_winograd_forward; any desc.tile but RESIDENT / HALF)
TILE_WINO_RES = 6         # ... its patch-resident variant (cin <= 96, many cout tiles)
TILE_PATCH = 7            # bf16 mode: the LDS-resident-patch 3x3 kernel (sgv3d_conv3x3_patch_bf16_forward)
TILE_WINO_HALF = 8        # ... 64 tiles x 32 channels per workgroup, positions split over wave pairs (2 workgroups / CU)
TILE_WINO4 = 9            # Winograd F(4x4,3x3) in three launches (sgv3d_conv2d_winograd4_forward), GEMM tile 64x64
TILE_WINO4_WIDE = 10      # ... 64x128
TILE_WINO4_NARROW = 15    # ... 32x128: rows per position padded to 32 instead of 64 (336 tiles -> 352, 84 -> 96)
TILE_F4RES = 40           # F(4x4,3x3) in ONE launch, the transformed input resident in LDS (sgv3d_conv3x3_f4res_forward)
TILE_WINO4_OCC = 46       # F(4x4) with the five-workgroups-per-CU form of the 64x64 GEMM tile
TILE_WINO4_G48 = 47       # F(4x4) with the grouped GEMM on v_mfma_f32_16x16x4_f32, 48 x 64 tiles: rows padded to 48 (336 -> 336)

# split-K policy classes: a split s of SPLITS is proposed when k-steps // s >= min_k, the unsplit grid has fewer than max_wgs
# workgroups and the split one at most max_total
SPLITS = (2, 3, 4, 6, 8)
SPLIT_POLICY = {"igemm": dict(min_k=4, max_wgs=2048, max_total=6144),
                "patch": dict(min_k=2, max_wgs=float("inf"), max_total=1024),
                "dw": dict(min_k=4, max_wgs=384, max_total=1024)}

Tile = namedtuple("Tile", "id label family entry abi form bm bn spatial split x3 mfirst occ5 deep only symbol flops")
TILES = {}


def _add(id, label, family, entry, abi, form, bm, bn, spatial=None, split=None, x3=False, mfirst=False, occ5=False, deep=False, only=None,
         symbol=None, flops=None):
    assert id not in TILES and (split is None or split in SPLIT_POLICY), id
    TILES[id] = Tile(id, label, family, entry, abi, form, bm, bn, spatial, split, x3, mfirst, occ5, deep, only, symbol, flops)


# implicit GEMM (csrc/conv_igemm.hip): sgv3d_conv2d_forward / _bf16 / _f32x3 / _bf16io by mode.  1..4, 11..14 = their f32x3 products,
# 21..24 = m-tile first, 44 / 45 = the 64x64 tile at five workgroups per CU (f32, channel-chunk-major weights; 45: m-tile first)
for _abi, (_bm, _bn) in ((SGV3D_TILE_128x128, (128, 128)), (SGV3D_TILE_128x64, (128, 64)), (SGV3D_TILE_64x128, (64, 128)),
                         (SGV3D_TILE_64x64, (64, 64))):
    _sym = dict(symbol=f"conv_igemm_kernel<{_bm // 64}, {_bn // 64}, {{chunk}}, false, {{pw}}, false, false>", flops="direct")
    for _base, _kw in ((0, _sym), (10, dict(x3=True, only="f32")), (20, dict(_sym, mfirst=True))):
        _add(_base + _abi, f"{_bm}x{_bn}", "igemm", "conv2d", _abi | (SGV3D_TILE_MFIRST if _base == 20 else 0), "w", _bm, _bn, split="igemm",
             **_kw)
for _id, _mf in ((44, 0), (45, SGV3D_TILE_MFIRST)):
    _add(_id, "64x64", "igemm", "conv2d", SGV3D_TILE_64x64 | SGV3D_TILE_OCC5 | _mf, "w", 64, 64, split="igemm", mfirst=bool(_mf), occ5=True,
         only="f32", symbol="conv_igemm_kernel<1, 1, {chunk}, false, {pw}, false, true>", flops="direct")
# Winograd F(2x2,3x3) (csrc/conv_wino.hip): 16 x 16 output pixels per workgroup
_add(TILE_WINO, "wino", "wino", "winograd", TILE_WINO, "w_wino", 256, 64, spatial=(16, 16, 4), split="igemm", only="f32")
_add(TILE_WINO_RES, "wino_resident", "wino", "winograd", SGV3D_WINOGRAD_RESIDENT, "w_wino", 256, 64, spatial=(16, 16, 4), only="f32")
_add(TILE_WINO_HALF, "wino_half", "wino", "winograd", SGV3D_WINOGRAD_HALF, "w_wino", 256, 32, spatial=(16, 16, 4), split="igemm", only="f32")
# bf16 mode: the LDS-resident-patch 3x3 kernel (csrc/conv_patch_bf16.hip): 16 x 32 output pixels per workgroup, stages of 32 channels
_add(TILE_PATCH, "patch_bf16", "patch_bf16", "patch_bf16", None, "w_patch", 512, 64, spatial=(16, 32, 32), split="patch", only="bf16")
# Winograd F(4x4,3x3) in three launches: the position GEMM is the implicit-GEMM kernel (pointwise form) or the grouped 16x16x4 GEMM
for _id, _abi, _bm, _bn, _sym in (
        (TILE_WINO4, SGV3D_TILE_64x64, 64, 64, "conv_igemm_kernel<1, 1, true, false, true, false, false>"),
        (TILE_WINO4_WIDE, SGV3D_TILE_64x128, 64, 128, "conv_igemm_kernel<1, 2, true, false, true, false, false>"),
        # (conv_igemm_kernel<1, 1, true, false, true, true, false>; never reported: profile records are kept as they were)
        (TILE_WINO4_NARROW, SGV3D_TILE_32x128, 32, 128, None),
        (TILE_WINO4_OCC, SGV3D_TILE_64x64 | SGV3D_TILE_OCC5, 64, 64, "conv_igemm_kernel<1, 1, true, false, true, false, true>"),
        (TILE_WINO4_G48, SGV3D_TILE_48x64, 48, 64, "gemm16_grouped_kernel<3>")):
    _add(_id, "wino4", "wino4", "winograd4", _abi, "w_wino4", _bm, _bn, only="f32", symbol=_sym, flops="wino4" if _sym else None)
# ... with the position GEMM on the bf16 matrix cores, f32-accurate (csrc/gemm_x3_grouped.hip: every operand split exactly into three
# bf16 terms by its PRODUCER -- the weight packer, the input transform --, six partial products accumulated in f32).  50 + v:
# v % 5 = m-tile of {48, 64, 96, 112, 128} rows, v >= 5: 160 instead of 128 columns per workgroup
for _v in range(10):
    _bm, _bn = (48, 64, 96, 112, 128)[_v % 5], 160 if _v >= 5 else 128
    _add(50 + _v, "wino4_x3", "wino4_x3", "winograd4", SGV3D_TILE_X3 | _v, "w_wino4_x3", _bm, _bn, x3=True, only="f32",
         symbol=f"gemm_x3_grouped_kernel<{_bm // 16}, {_bn // 32}>", flops="wino4")
# F(4x4,3x3) in ONE launch with V = B^T d B of a 16x16 block resident in LDS (csrc/head_wino4.hip: conv_f4res_kernel)
_add(TILE_F4RES, "wino4_resident", "f4res", "f4res", None, "w_f4res", 256, 64, only="f32")
# implicit GEMM with f32x3 products (csrc/conv_pw_x3.hip: weights split into three bf16 terms by the packer, activations on their way
# into LDS).  variant & 3 = {0: 32, 1: 64, 2: 128} pixels per workgroup, variant & 4: 64 instead of 128 channels, variant | 8: 256
# channels (8 waves); host ids 60 + v, 70 + v = m-tile first, 80 + v / 90 + v (m-tile first) = variant 8 + v
for _base, _var0, _mf in ((60, 0, 0), (70, 0, SGV3D_TILE_MFIRST), (80, 8, 0), (90, 8, SGV3D_TILE_MFIRST)):
    for _v in (0, 1, 2) + ((4, 5, 6) if _var0 == 0 else ()):
        _bm, _bn = 32 << (_v & 3), 256 if _var0 else 64 if _v & 4 else 128
        _add(_base + _v, "pw_x3", "pw_x3", "x3", SGV3D_TILE_X3 | (_var0 + _v) | _mf, "w_pw_x3", _bm, _bn, split="igemm", x3=True,
             mfirst=bool(_mf), only="f32", symbol=f"conv_pw_x3_kernel<{_bm // 16}, {_bn // 32}, {{kmode}}>", flops="direct_k32")
# bf16 mode, bf16 tensors in and out: the direct-weight implicit GEMM (sgv3d_conv_dw_bf16_forward), pixels x channels per workgroup
# 64x256 / 128x128 / 256x64 (64 pixels per wave), 128x256 / 256x128 (128 pixels per wave), 64x128 (one 32-channel tile per wave: twice
# the workgroups of 64x256 on small maps).  *_DEEP: for launches of about one workgroup per CU, where nothing else hides the memory
# round trips; no split-K
for _abi, _bm, _bn, _deep in ((SGV3D_TILE_DW_64x256, 64, 256, False), (SGV3D_TILE_DW_128x128, 128, 128, False),
                              (SGV3D_TILE_DW_256x64, 256, 64, False), (SGV3D_TILE_DW_128x256, 128, 256, False),
                              (SGV3D_TILE_DW_256x128, 256, 128, False), (SGV3D_TILE_DW_64x256_DEEP, 64, 256, True),
                              (SGV3D_TILE_DW_128x128_DEEP, 128, 128, True), (SGV3D_TILE_DW_64x128, 64, 128, False),
                              (SGV3D_TILE_DW_64x128_DEEP, 64, 128, True)):
    _add(_abi, "dw_bf16", "dw_bf16", "dw_bf16", _abi, "w_dw", _bm, _bn, split=None if _deep else "dw", deep=_deep, only="bf16")

TILES = dict(sorted(TILES.items()))
FAMILIES = ("igemm", "wino", "wino4", "wino4_x3", "f4res", "pw_x3", "patch_bf16", "dw_bf16")
assert {t.family for t in TILES.values()} == set(FAMILIES)


def select(*families, **flags):
    """Ids (ascending) of the given families whose x3 / mfirst / occ5 / deep flags are as given (default False)."""
    want = dict(dict(x3=False, mfirst=False, occ5=False, deep=False), **flags)
    return tuple(t.id for t in TILES.values() if t.family in families and all(getattr(t, k) == v for k, v in want.items()))


def family(*families):
    """Every id (ascending) of the given families."""
    return tuple(t.id for t in TILES.values() if t.family in families)


def by_shape(fam, bm, bn, deep=False):
    """The id of the family's tile with this workgroup footprint."""
    (t,) = (t.id for t in TILES.values() if t.family == fam and (t.bm, t.bn, t.deep) == (bm, bn, deep))
    return t
