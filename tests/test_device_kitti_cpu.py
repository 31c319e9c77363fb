"""CPU: the host side of the device detection -> KITTI annotation path (csrc/result2kitti.hip): the C ABI and its
argument checks, the decimal rounding against CPython's ``round``, the restatement of ``_format_bbox`` + ``_convert``
through the host entry against the reference's own label files (tests/golden/result2kitti.npz) and against the file
chain on seeded random detections.  The kernel runs the same per-detection function (test_device_kitti_gpu.py)."""
import ctypes
import json
import math
import os
import random
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import kitti_chain_util as U
from conftest import ROOT
from sgv3d_amd import _lib

R2K = U.R2K
NEW = ("sgv3d_round_decimals_host", "sgv3d_detections_to_kitti_workspace_bytes", "sgv3d_detections_to_kitti",
       "sgv3d_detections_to_kitti_host")
_CTYPE = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


def _header_proto(name):
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"([a-z_0-9]+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in sgv3d_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const ", "").split()[0]])
    return _CTYPE[m.group(1)], args


@pytest.mark.parametrize("name", NEW)
def test_header_and_ctypes_agree(name):
    res, args = _header_proto(name)
    assert name in _lib.EXPORTED_SYMBOLS
    assert _lib._PROTOS[name] == (res, args)
    assert hasattr(_lib.load(), name)


def _good_args(device):
    """A complete, valid argument list over small host arrays (kept alive by the caller) for either entry."""
    B, N, M = 2, 4, 3
    a = dict(boxes=np.zeros((B, N, 9), np.float32), scores=np.zeros((B, N), np.float32), labels=np.zeros((B, N), np.int32),
             counts=np.zeros(B, np.int32), calib=np.zeros((B, 33)), table=U.TABLE.copy(), work=np.zeros(B * N, np.int32),
             fields=np.zeros((B, M, 13)), cls=np.zeros((B, M), np.int32), kept=np.zeros(B, np.int32))
    P = lambda k: a[k].ctypes.data
    args = dict(batch=B, n=N, boxes=P('boxes'), scores=P('scores'), f64=0, labels=P('labels'), counts=P('counts'), calib=P('calib'),
                table=P('table'), num_classes=len(U.TABLE), thr=0.45, w=1920, h=1080, max_det=M, digits=4)
    if device:
        args.update(work=P('work'), work_bytes=B * N * 4)
    args.update(fields=P('fields'), cls=P('cls'), kept=P('kept'))
    if device:
        args.update(stream=None)
    return a, args


@pytest.mark.parametrize("device", [False, True], ids=["host_entry", "device_entry"])
def test_every_bad_argument_is_refused_before_any_launch(device):
    """Each call below has exactly one bad argument, so none reaches the launch (there is no GPU here)."""
    lib = _lib.load()
    fn = lib.sgv3d_detections_to_kitti if device else lib.sgv3d_detections_to_kitti_host
    keep, good = _good_args(device)
    bad = [(k, None) for k in ('boxes', 'scores', 'labels', 'counts', 'calib', 'table', 'fields', 'cls', 'kept')]
    bad += [('batch', 0), ('batch', -1), ('n', 0), ('max_det', 0), ('max_det', -5), ('digits', 3), ('digits', 0), ('digits', -2),
            ('num_classes', 0), ('num_classes', 65), ('f64', 2), ('w', 0), ('h', -1)]
    if device:
        bad += [('work', None)]
    for key, value in bad:
        rc = fn(*dict(good, **{key: value}).values())
        assert rc == -1, (key, value, rc)                                    # SGV3D_EINVAL
        assert lib.sgv3d_last_error(), key
    keep['table'][2] = 3                                                     # not a KITTI class id
    assert fn(*good.values()) == -1 and b"class_table" in lib.sgv3d_last_error()
    keep['table'][2] = -1
    if device:
        need = lib.sgv3d_detections_to_kitti_workspace_bytes(good['batch'], good['n'])
        assert need == good['batch'] * good['n'] * 4
        rc = fn(*dict(good, work_bytes=need - 1).values())
        assert rc == -3 and b"workspace" in lib.sgv3d_last_error()           # SGV3D_ENOSPACE
        assert fn(*dict(good, work=good['work'] + 2).values()) == -1 and b"misaligned" in lib.sgv3d_last_error()
        assert lib.sgv3d_detections_to_kitti_workspace_bytes(0, 4) == 0 and lib.sgv3d_detections_to_kitti_workspace_bytes(2, 0) == 0
    else:
        assert fn(*good.values()) == 0                                       # the list itself is valid
    assert math.isnan(lib.sgv3d_round_decimals_host(1.0, 3)) and b"digits" in lib.sgv3d_last_error()
    assert lib.sgv3d_round_decimals_host(0.123456789, -1) == 0.123456789


# ------------------------------------------------------------------------------------------------------------ rounding
def _bits(v):
    return struct.pack('<d', v)


def _rounding_values():
    rnd = random.Random(20240607)
    vals = [0.45, 1920.0, 1080.0, 0.0, -0.0, -1e-5, 1e-5, float(np.float32(0.45))]
    vals += [rnd.uniform(-2e3, 2e3) for _ in range(60000)]
    vals += [rnd.choice((-1, 1)) * rnd.random() * 10.0 ** rnd.randint(-12, 3) for _ in range(40000)]      # sixteen decades
    ties = [(k + 0.5) / 1e4 for k in range(-40000, 40000)]                       # every decimal tie to +-4: (k + 0.5) * 1e-4
    ties += [s * (k + m / 2.0 ** e) for s in (-1, 1) for k in range(4) for e in range(5, 14) for m in range(1, 2 ** e, 2)
             if (Fraction(m, 2 ** e) * 10 ** 4 % 1) == Fraction(1, 2)]           # exact dyadic ties: 0.03125, 0.09375, ...
    assert 0.03125 in ties
    for t in ties:
        lo1, hi1 = math.nextafter(t, -math.inf), math.nextafter(t, math.inf)
        vals += [t, lo1, hi1, math.nextafter(lo1, -math.inf), math.nextafter(hi1, math.inf)]
    return vals


def test_round_decimals_is_cpythons_round_bit_for_bit():
    f = _lib.load().sgv3d_round_decimals_host
    vals = _rounding_values()
    assert len(vals) > 500000
    wrong = [(v, f(v, 4), round(v, 4)) for v in vals if _bits(f(v, 4)) != _bits(round(v, 4))]
    assert not wrong, (len(wrong), wrong[:5])
    assert _bits(f(-1e-5, 4)) == _bits(-0.0) and _bits(f(-0.0, 4)) == _bits(-0.0) and _bits(f(0.0, 4)) == _bits(0.0)
    # np.round is a different function on the dyadic ties whose product with 1e4 is exact
    assert f(0.03125, 4) == round(0.03125, 4) == 0.0312 and f(0.12345, 4) == 0.1235 != float(np.round(0.12345, 4))


# --------------------------------------------------------------------------------------------------------- golden text
def _fixture_arrays(results_json, toks):
    """The fixture's JSON records as float64 arrays (box = x, y, z, l, w, h, yaw; size in the JSON is (w, l, h))."""
    res = json.loads(str(results_json))['results']
    n = max(len(res[t]) for t in toks)
    boxes, scores = np.zeros((len(toks), n, 9)), np.zeros((len(toks), n))
    labels, counts = np.zeros((len(toks), n), np.int32), np.zeros(len(toks), np.int32)
    for b, t in enumerate(toks):
        counts[b] = len(res[t])
        for i, p in enumerate(res[t]):
            w, l, h = p['size']
            boxes[b, i, :7] = list(p['translation']) + [l, w, h, p['box_yaw']]
            scores[b, i] = p['detection_score']
            labels[b, i] = U.CLASS_NAMES.index(p['detection_name'])
    return boxes, scores, labels, counts


def _layout_calibs(layout, tmp_path):
    if layout == 'kitti':
        return U.fixture_calibs(U.kitti_root(tmp_path)), U.tokens(), U.GOLD['results_json'], U.GOLD['label_text']
    if layout == 'dair':
        root = tmp_path / 'dair-v2x-i'
        for sub in ('camera_intrinsic', 'virtuallidar_to_camera'):
            os.makedirs(root / 'calib' / sub)
        for sid, cam, v2c in zip(U.GOLD['calib_ids'], U.GOLD['dair_cam_json'], U.GOLD['dair_v2c_json']):
            (root / 'calib' / 'camera_intrinsic' / f'{int(sid):06d}.json').write_text(str(cam))
            (root / 'calib' / 'virtuallidar_to_camera' / f'{int(sid):06d}.json').write_text(str(v2c))
        calibs = [R2K.load_calib_dair_json(str(root), int(sid)) for sid in U.GOLD['calib_ids']]
        return calibs, U.tokens(), U.GOLD['results_json'], U.GOLD['dair_label_text']
    root = tmp_path / 'rope3d'
    for tok, split, den, cal in zip(U.GOLD['rope_tokens'], U.GOLD['rope_split'], U.GOLD['rope_denorm_text'], U.GOLD['rope_calib_text']):
        for sub, text in (('denorm', den), ('calib', cal)):
            os.makedirs(root / str(split) / sub, exist_ok=True)
            (root / str(split) / sub / f'{tok}.txt').write_text(str(text))
    toks = [str(t) for t in U.GOLD['rope_tokens']]
    return [R2K.load_calib_rope3d(str(root), t) for t in toks], toks, U.GOLD['rope_results_json'], U.GOLD['rope_label_text']


@pytest.mark.parametrize("layout", ["kitti", "dair", "rope3d"])
def test_host_entry_writes_the_reference_label_text(layout, tmp_path):
    """The reference's own output pins the restatement: KITTI files (float32 rows), DAIR JSON (float64), Rope3D (denorm).
    The JSON's numbers are doubles, so they go in as doubles (f64_inputs = 1)."""
    calibs, toks, results_json, want = _layout_calibs(layout, tmp_path)
    boxes, scores, labels, counts = _fixture_arrays(results_json, toks)
    calib = U.calib_blocks(calibs, U.metas_for(toks))
    kept, cls, fields = U.host_entry(boxes, scores, labels, counts, calib, boxes.shape[1], 4)
    lines = 0
    for b in range(len(toks)):
        assert U.format_rows(cls[b, :kept[b]], fields[b, :kept[b]]) == str(want[b]), (layout, b)
        lines += int(kept[b])
    assert lines >= 8 and lines < counts.sum()                       # the fixture keeps detections and drops others


# ----------------------------------------------------------------------------------------------- against the file chain
@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """Seeded random detections through the file chain, once: rounded and unrounded label rows per sample."""
    tmp = tmp_path_factory.mktemp("chain")
    root = U.kitti_root(tmp)
    det = U.random_detections(3, 96, (0, 17, 96), seed=11)
    metas = U.metas_for(U.tokens())
    rounded = U.file_chain(U.as_results(*det), metas, root, tmp / 'rounded')
    with U.unrounded():
        exact = U.file_chain(U.as_results(*det), metas, root, tmp / 'exact')
    ids = [int(s) for s in U.GOLD['calib_ids']]
    return dict(det=det, calib=U.calib_blocks(U.fixture_calibs(root), metas), rounded=[U.read_rows(rounded, i) for i in ids],
                exact=[U.read_rows(exact, i) for i in ids])


def test_unrounded_fields_and_keep_rule_match_the_file_chain(chain):
    boxes, scores, labels, counts = chain['det']
    kept, cls, fields = U.host_entry(boxes, scores, labels, counts, chain['calib'], 96, -1)
    worst, total = 0.0, 0
    for b in range(3):
        want_cls, want = chain['exact'][b]
        # the keep rule restated in numpy: order, classes and count
        ok = (scores[b, :counts[b]].astype(np.float64) > 0.45) & (U.TABLE[labels[b, :counts[b]]] >= 0)
        assert kept[b] == ok.sum() == len(want_cls)
        assert np.array_equal(cls[b, :kept[b]], want_cls) and np.array_equal(want_cls, U.TABLE[labels[b, :counts[b]]][ok])
        assert np.array_equal(fields[b, :kept[b], 12], scores[b, :counts[b]][ok].astype(np.float64))     # input order, compacted
        assert np.all(cls[b, kept[b]:] == -7) and np.all(np.isnan(fields[b, kept[b]:]))                  # nothing else written
        if kept[b]:
            worst = max(worst, float(np.abs(fields[b, :kept[b]] - want).max()))
        total += int(kept[b])
    print(f"unrounded: max |host - file chain| = {worst:.3e} over {total} rows")
    assert kept[0] == 0 and total >= 40
    # a-priori: about 40 operations x 2^-53 x 2e3 ~ 1e-11 plus 2 ulp per libm call; the bar is two decades over it
    assert worst <= 1e-9
    # float32(0.45) is below 0.45 as a double: counted among the inputs, never kept; the next float32 above it is kept
    at, above = float(np.float32(0.45)), float(np.nextafter(np.float32(0.45), np.float32(1)))
    assert at < 0.45 < above and (scores[2] == np.float32(0.45)).sum() >= 5
    assert not np.any(fields[2, :kept[2], 12] == at) and np.any(fields[2, :kept[2], 12] == above)
    assert set(labels[2].tolist()) == set(range(10))


def test_rounded_fields_match_the_file_chain_away_from_boundaries(chain):
    boxes, scores, labels, counts = chain['det']
    kept, cls, fields = U.host_entry(boxes, scores, labels, counts, chain['calib'], 96, 4)
    got = np.concatenate([fields[b, :kept[b]] for b in range(3)])
    want = np.concatenate([chain['rounded'][b][1] for b in range(3)])
    exact = np.concatenate([chain['exact'][b][1] for b in range(3)])
    assert got.shape == want.shape == exact.shape
    # the file chain alone: its own share of values near a boundary stays under the cap for this seed
    assert (U.boundary_distance(exact) <= U.BOUNDARY).mean() <= U.CAP
    share = U.assert_rounded_alike(got, want, exact)
    print(f"rounded: {share * 100:.3f} % of {got.size} values within {U.BOUNDARY} of a boundary")


def test_ego2global_moves_the_location_and_not_rotation_y(tmp_path):
    """A 90 degree turn about z plus a translation: ``location`` follows the moved centre, ``rotation_y`` is still
    pi/2 - yaw of the raw box, as in the file chain (``box_yaw`` is the raw yaw)."""
    root = U.kitti_root(tmp_path)
    det = U.random_detections(3, 24, (24, 5, 0), seed=5)
    det[0][..., 0], det[0][..., 1] = det[0][..., 1].copy(), -det[0][..., 0].copy()          # turned back by the ego2global turn
    rot, trans = (math.cos(math.pi / 4), 0.0, 0.0, math.sin(math.pi / 4)), (1.0, 2.0, 0.25)
    metas, plain = U.metas_for(U.tokens(), rot, trans), U.metas_for(U.tokens())
    with U.unrounded():
        exact = U.file_chain(U.as_results(*det), metas, root, tmp_path / 'exact')
    calibs = U.fixture_calibs(root)
    kept, cls, fields = U.host_entry(*det, U.calib_blocks(calibs, metas), 24, -1)
    kept0, _, fields0 = U.host_entry(*det, U.calib_blocks(calibs, plain), 24, -1)
    assert np.array_equal(kept, kept0) and kept[0] >= 5
    for b, sid in enumerate(U.GOLD['calib_ids']):
        want_cls, want = U.read_rows(exact, sid)
        assert np.array_equal(cls[b, :kept[b]], want_cls)
        if kept[b]:
            assert np.abs(fields[b, :kept[b]] - want).max() <= 1e-9
    m = kept[0]
    assert np.array_equal(fields[0, :m, 11], fields0[0, :m, 11])                             # rotation_y: untouched
    assert np.abs(fields[0, :m, 8:11] - fields0[0, :m, 8:11]).min() > 1.0                    # location: moved
    # the moved centre itself: Tr . (Rz(90) . c + t)
    Tr = calibs[0][0]
    c = det[0][0, :det[3][0], :3].astype(np.float64)
    ok = (det[1][0, :det[3][0]].astype(np.float64) > 0.45) & (U.TABLE[det[2][0, :det[3][0]]] >= 0)
    moved = np.stack([-c[:, 1], c[:, 0], c[:, 2]], 1) + np.array(trans)
    assert np.abs((moved[ok] @ Tr[:3, :3].T + Tr[:3, 3]) - fields[0, :m, 8:11]).max() < 1e-9
