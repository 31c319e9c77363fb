"""The device AP evaluator without a GPU: the C ABI's declarations and rejections, and the host twin
(``sgv3d_kitti_eval_device_host``: the functions the kernels run, lanes as a loop) against the host path's own parts --
``clean_data`` + ``sgv3d_kitti_eval_curves`` per cell --, the reference's goldens and the oracle's recall thresholds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import device_eval_util as U
from conftest import ROOT
from oracle import kitti_eval_ref as R
from sgv3d_amd import _lib
from sgv3d_amd.evaluators import device_eval as DE
from sgv3d_amd.evaluators.kitti_utils.eval import kitti_eval

ENTRIES = ("sgv3d_kitti_eval_device_workspace_bytes", "sgv3d_kitti_eval_device", "sgv3d_kitti_eval_device_host")


def test_header_and_ctypes_agree_on_the_new_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_lib._PROTOS[name][1]), name
        assert hasattr(lib, name)


def _call(lib, which, **over):
    """One call with valid arguments except ``over``; no launch can happen: every pointer is host memory and every case
    here is refused before the first launch."""
    gts, dts = U.stress_set(0, images=3)
    pk = DE.pack_annotations(gts, dts)
    C = 2
    a = dict(M=pk.M, TG=pk.TG, TD=pk.TD, pairs=pk.pairs, tiles=pk.tiles, packed=pk.buffer.data_ptr(), nbytes=pk.buffer.numel(), C=C,
             classes=np.array([0, 3], np.int32), mo=np.ascontiguousarray(U.MIN_OVERLAPS[:, :, [0, 3]]), aos=1,
             out=np.zeros(18 * C * 41 * 3 + 64), ws=np.zeros(8), ws_bytes=64)
    a.update(over)
    o = a['out'].ctypes.data
    n = 18 * C * 41 * 8
    ptr = lambda v: v if v is None or isinstance(v, int) else v.ctypes.data
    outs = [o, o + n, o + 2 * n, o + 3 * n, o + 3 * n + 18 * C * 4]
    for k, key in enumerate(('precision', 'recall', 'orientation', 'nthr', 'status')):
        if key in over:
            outs[k] = over[key]
    if which == 'host':
        ov = np.zeros(max(pk.pairs, 1), np.float32)
        return lib.sgv3d_kitti_eval_device_host(a['M'], a['TG'], a['TD'], a['pairs'], a['packed'], a['nbytes'], ov.ctypes.data, ov.ctypes.data,
                                                a['C'], ptr(a['classes']), ptr(a['mo']), a['aos'], *outs, None)
    return lib.sgv3d_kitti_eval_device(a['M'], a['TG'], a['TD'], a['pairs'], a['tiles'], a['packed'], a['nbytes'], a['C'], ptr(a['classes']),
                                       ptr(a['mo']), a['aos'], ptr(a['ws']), a['ws_bytes'], *outs, None)


@pytest.mark.parametrize("which", ["host", "device"])
def test_rejections_without_a_gpu(which):
    lib = _lib.load()
    bad_mo = np.ascontiguousarray(U.MIN_OVERLAPS[:, :, [0, 3]]).copy()
    bad_mo[1, 2, 1] = -0.25
    cases = [(dict(M=-1), b"negative count"), (dict(TG=-1), b"negative count"), (dict(TD=-1), b"negative count"),
             (dict(pairs=-1), b"negative count"), (dict(packed=None), b"null pointer"), (dict(classes=None), b"null pointer"),
             (dict(mo=None), b"null pointer"), (dict(precision=None), b"null pointer"), (dict(status=None), b"null pointer"),
             (dict(C=0), b"num_classes"), (dict(C=5), b"num_classes"), (dict(classes=np.array([0, 4], np.int32)), b"class id 4"),
             (dict(classes=np.array([-1, 2], np.int32)), b"class id -1"), (dict(mo=bad_mo), b"minimum overlap"),
             (dict(nbytes=24), b"packed input"), (dict(aos=2), b"compute_aos"), (dict(TG=5), b"packed input"),
             (dict(M=0), b"in no image"), (dict(TG=(1 << 28) + 1), b"out of range")]
    for over, message in cases:
        assert _call(lib, which, **over) == -1, over
        assert message in lib.sgv3d_last_error(), (over, lib.sgv3d_last_error())
    if which == 'device':
        assert _call(lib, which, ws=None) == -1 and b"workspace" in lib.sgv3d_last_error()
        assert _call(lib, which, tiles=-1) == -1
        # a short workspace is its own code, and comes before any launch (these are host pointers)
        assert _call(lib, which, ws_bytes=64) == -3 and b"needed" in lib.sgv3d_last_error()
    else:
        assert _call(lib, which) == 0


def test_workspace_bytes():
    lib = _lib.load()
    f = lib.sgv3d_kitti_eval_device_workspace_bytes
    assert f(-1, 1, 1, 1, 3) == 0 and f(1, -1, 1, 1, 3) == 0 and f(1, 1, 1, 2, 3) == 0 and f(1, 1, 1, 1, 0) == 0 and f(1, 1, 1, 1, 5) == 0
    small, big = f(2, 1000, 10, 5000, 3), f(2, 1025, 10, 5000, 3)
    assert small % 8 == 0 and big - small >= 54 * 1024 * 8          # the slots double across the 1024 padding
    assert f(0, 0, 0, 0, 1) > 0 and f(0, 3, 0, 0, 1) == 0 and f(1, (1 << 28) + 1, 1, 1, 1) == 0


def test_kitti_eval_device_raises_without_a_gpu():
    gts, dts = U.golden_annos()
    with pytest.raises(RuntimeError, match="no CPU path"):
        DE.kitti_eval_device(gts, dts, ['Car'], device='cpu')
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            DE.kitti_eval_device(gts, dts, ['Car'])


def test_packing_refuses_what_the_kernels_cannot_rank():
    gts, dts = U.stress_set(1, images=2)
    dts[1]['score'] = dts[1]['score'].copy()
    if len(dts[1]['score']) == 0:
        dts[1] = U._anno(np.random.default_rng(0), 3, U.DT_NAMES, True)
    dts[1]['score'][0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        DE.pack_annotations(gts, dts)
    packed = DE.pack_ground_truth(gts)
    assert DE.pack_ground_truth(packed) is packed and DE.pack_ground_truth(gts) is not packed      # a snapshot, handed over as it is


def _crowded(extra=1):
    """Three images; the middle one has ``MAX_DETECTIONS + extra`` detections."""
    gts, dts = U.stress_set(2, images=3)
    gts[1] = U._anno(np.random.default_rng(5), 7, U.GT_NAMES, False)
    dts[1] = U._anno(np.random.default_rng(6), DE.MAX_DETECTIONS + extra, U.DT_NAMES, True)
    return gts, dts


def test_more_than_4096_detections_in_an_image_are_refused(monkeypatch):
    """The host path has no such limit; here it is refused by name: in ``pack_annotations``, and in the host twin for a
    caller that packs by other means.  4096 itself is matched."""
    gts, dts = _crowded()
    with pytest.raises(ValueError, match="at most 4096"):
        DE.pack_annotations(gts, dts)
    monkeypatch.setattr(DE, 'MAX_DETECTIONS', 1 << 20)                 # pack what the library refuses
    pk = DE.pack_annotations(gts, dts)
    zeros = np.zeros(pk.pairs, np.float32)
    with pytest.raises(_lib.SGV3DError, match="4097 detections"):
        DE.curves_host(pk, zeros, zeros, [0], U.MIN_OVERLAPS[:, :, [0]], False)
    monkeypatch.undo()
    gts, dts = _crowded(extra=0)
    bev, d3 = U.random_overlaps(9, gts, dts)
    classes = [0, 1]
    got = DE.curves_host(DE.pack_annotations(gts, dts), bev, d3, classes, U.MIN_OVERLAPS[:, :, classes], True)
    assert got[4] == 0
    U.assert_curves(got, U.yardstick_curves(gts, dts, classes, U.MIN_OVERLAPS[:, :, classes], bev, d3, True))


@pytest.mark.parametrize("seed", range(6))
def test_host_twin_matches_the_curve_function_on_random_frames(seed):
    """Precomputed rotated overlaps rounded to 0.1, tied scores, empty images, every ignore flag, DontCare boxes, and
    detection counts 0, 1, 63, 64, 65, 130 against ground-truth counts 0, 1, 7, 65."""
    gts, dts = U.stress_set(seed)
    assert {len(d['name']) for d in dts} >= set(U.DT_COUNTS) and {len(g['name']) for g in gts} >= set(U.GT_COUNTS)
    bev, d3 = U.random_overlaps(seed, gts, dts)
    classes = [[0, 1, 2, 3], [3, 0], [1], [2, 1, 0]][seed % 4]
    mo = U.MIN_OVERLAPS[:, :, classes]
    aos = seed % 3 != 2
    want = U.yardstick_curves(gts, dts, classes, mo, bev, d3, aos)
    got = DE.curves_host(DE.pack_annotations(gts, dts), bev, d3, classes, mo, aos)
    assert got[4] == 0
    U.assert_curves(got, want)
    assert want[3].max() > 3 and (want[0] > 0).any()
    if not aos:
        assert not got[2].any()


def test_host_twin_derives_the_flags_of_every_name_kind():
    """Annotation dicts with every name kind (Van, Person_sitting, DontCare, lower-case dontcare, other spellings) and a
    class that no box carries: the twin's own flags and 2-D overlaps against clean_data + the curve function."""
    gts, dts = U.stress_set(40, images=10)
    names = {str(n) for g in gts for n in g['name']}
    assert names >= {'Van', 'Person_sitting', 'DontCare', 'dontcare', 'car', 'Truck'}
    for g in gts:                                               # no Bus in the set: class 3 is absent
        g['name'] = np.array(['Truck' if n == 'Bus' else n for n in g['name']], dtype=str) if len(g['name']) else g['name']
    for d in dts:
        d['name'] = np.array(['Truck' if n == 'Bus' else n for n in d['name']], dtype=str) if len(d['name']) else d['name']
    bev, d3 = U.random_overlaps(40, gts, dts)
    classes = [0, 1, 2, 3]
    want = U.yardstick_curves(gts, dts, classes, U.MIN_OVERLAPS, bev, d3, True)
    got = DE.curves_host(DE.pack_annotations(gts, dts), bev, d3, classes, U.MIN_OVERLAPS, True)
    U.assert_curves(got, want)
    assert not want[3][:, 3].any() and want[3][:, :3].any(axis=(0, 2, 3)).all()
    # the name ids are what the flags come from
    ids = DE.name_ids(['Car', 'car', 'Van', 'Person_sitting', 'DontCare', 'dontcare', 'Bus', 'Tram'])
    assert ids.tolist() == [0, 0, 4, 5, 6 | 8, 6, 3, 6]


def test_host_twin_matches_the_reference_goldens():
    gts, dts = U.golden_annos()
    classes = [0, 1, 2]
    mo = U.MIN_OVERLAPS[:, :, classes]
    got = DE.curves_host(DE.pack_annotations(gts, dts), U.flat_overlaps(gts, dts, 1), U.flat_overlaps(gts, dts, 2), classes, mo, True)
    assert got[4] == 0
    for m in range(3):
        np.testing.assert_allclose(got[0][m], U.GOLD[f'curve{m}_precision'], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(got[1][m], U.GOLD[f'curve{m}_recall'], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got[2][0], U.GOLD['curve0_orientation'], rtol=0, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("count", [0, 1, 2, 40, 41, 1023, 1024, 1025])
def test_recall_thresholds_are_the_oracles_bit_for_bit(count):
    """``count`` true positives in the Car cells (one box and one exact detection per image, plus two images that
    contribute none): fewer than 41 thresholds, exactly 41, and both sides of the sort's 1024 padding."""
    rng = np.random.default_rng(count)
    scores = np.round(rng.uniform(0.01, 1, count), 2)                     # ties
    box = np.array([[10.0, 10.0, 110.0, 100.0]])
    def anno(name, score):
        return {'name': np.array([name]), 'truncated': np.zeros(1), 'occluded': np.zeros(1), 'alpha': np.zeros(1), 'bbox': box.copy(),
                'dimensions': np.array([[4.0, 1.5, 1.8]]), 'location': np.array([[0.0, 1.0, 20.0]]), 'rotation_y': np.zeros(1),
                'score': np.array([score])}
    gts = [anno('Car', 0.0) for _ in range(count)] + [anno('Car', 0.0), anno('Truck', 0.0)]
    dts = [anno('Car', s) for s in scores] + [anno('Pedestrian', 0.9), anno('Car', 0.5)]
    ones = np.ones(count + 2, np.float32)
    thr = np.full((3, 1, 3, 2, 41), np.nan)
    got = DE.curves_host(DE.pack_annotations(gts, dts), ones, ones, [0], U.MIN_OVERLAPS[:, :, [0]], False, thresholds=thr)
    want = np.asarray(R.recall_thresholds(scores, count + 1), np.float64)
    assert got[4] == 0 and len(want) <= 41
    for cell in np.ndindex(3, 1, 3, 2):
        assert got[3][cell] == len(want)
        assert thr[cell][:len(want)].tobytes() == want.tobytes(), cell
        assert not thr[cell][len(want):].any()


def test_the_shared_report_helper_keeps_kitti_evals_text(monkeypatch):
    """``kitti_eval`` is ``eval_setup`` + ``do_eval`` + ``eval_report`` now: on the goldens, with the overlaps of the oracle in
    place of the GPU kernel's, its text and values are the reference's."""
    from sgv3d_amd.evaluators.kitti_utils import eval as E
    monkeypatch.setattr(E, 'calculate_overlaps', lambda g, d, metric: [R.frame_overlaps(a, b, metric) for a, b in zip(g, d)])
    gts, dts = U.golden_annos()
    text, ret = kitti_eval(gts, dts, ['Car', 'Pedestrian', 'Cyclist'])
    assert text == str(U.GOLD['result_text'])
    assert sorted(str(k) for k in U.GOLD['ret_keys']) == sorted(ret)
    np.testing.assert_allclose([ret[str(k)] for k in U.GOLD['ret_keys']], U.GOLD['ret_vals'], rtol=0, atol=1e-9)
