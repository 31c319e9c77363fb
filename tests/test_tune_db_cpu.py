"""CPU: the committed per-layer choices (tune/gfx950_*.json) only name algorithms this build knows."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_tune_dbs_name_known_tiles():
    from sgv3d_amd import conv_tiles
    files = sorted(glob.glob(os.path.join(ROOT, "tune", "gfx950_*.json")))
    assert files, "no committed tune DBs"
    tiles = conv_tiles.TILES
    for f in files:
        db = json.load(open(f))
        assert db, f
        for sig, choice in db.items():
            assert isinstance(choice, list) and len(choice) == 2, (f, sig, choice)
            t, s = int(choice[0]), int(choice[1])
            if sig.startswith("centerhead_branches"):
                assert t in (100, 101, 102), (f, sig, choice)            # fused F(2x2) / two kernels / fused F(4x4)
            elif sig.startswith("wgrad|"):
                assert t >= 0 and s >= 0, (f, sig, choice)               # weight-gradient (tile, pixel split); 0 = the kernel's own rule
                if sig.endswith("xbf16"):
                    assert t in (0, 1, 4, 6), (f, sig, choice)           # bf16 weight gradients: 64x64 / 128x128 per tap, 6 = all taps (3x3)
            elif sig.startswith("pair|"):
                assert t in (0, 1), (f, sig, choice)                     # fused conv2 + conv3 launch or not
            else:
                assert t in tiles and s >= 1, (f, sig, choice)
                assert tiles[t].only in (None, "bf16" if "bf16" in sig else "f32"), (f, sig, choice)    # bf16-only kernels / f32-only algorithms
                assert s == 1 or tiles[t].split is not None, (f, sig, choice)


def test_the_tile_table_is_what_hip_ops_exports():
    from sgv3d_amd import conv_tiles, hip_ops
    assert len(conv_tiles.TILES) == 61
    for t, T in conv_tiles.TILES.items():
        assert T.id == t and T.label and T.family in conv_tiles.FAMILIES and T.form and T.bm > 0 and T.bn > 0, T
        assert callable(getattr(hip_ops.PackedConv, "_launch_" + T.entry)) and T.form in hip_ops._FORMS, T
        assert (T.symbol is None) == (T.flops is None), T
    assert hip_ops.TILE_NAMES == {t: T.label for t, T in conv_tiles.TILES.items()}
    # the flags the committed-choice test relies on, id by id
    assert {t for t, T in conv_tiles.TILES.items() if T.only == "bf16"} == set(range(31, 40)) | {7}
    assert {40, 44, 45, 46, 47, 5, 6, 8, 9, 10, 15} <= {t for t, T in conv_tiles.TILES.items() if T.only == "f32"}
    assert {t for t, T in conv_tiles.TILES.items() if T.only is None} == {1, 2, 3, 4, 21, 22, 23, 24}


def test_every_candidate_tile_has_a_name():
    from sgv3d_amd import hip_ops
    for t in (hip_ops.TILE_WINO, hip_ops.TILE_WINO_RES, hip_ops.TILE_PATCH, hip_ops.TILE_WINO_HALF, hip_ops.TILE_F4RES) \
            + hip_ops.WINO4_TILES + hip_ops.DW_TILES + hip_ops.OCC5_TILES + (1, 2, 3, 4, 21, 22, 23, 24):
        assert t in hip_ops.TILE_NAMES, t
