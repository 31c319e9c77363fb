"""Shared by test_device_eval_cpu.py and test_device_eval_gpu.py: annotation sets small enough for seconds and shaped
so that the device match can go wrong on them, and the yardstick curves assembled per cell from ``clean_data`` +
``sgv3d_kitti_eval_curves`` (the host path's own parts)."""
import ctypes
import os

import numpy as np

from oracle import kitti_eval_ref as R
from sgv3d_amd import _lib
from sgv3d_amd.evaluators.kitti_utils.eval import clean_data, image_box_overlap

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "kitti_eval.npz"))
# kitti_eval's minimum overlaps [strict | loose, metric, class id]
MIN_OVERLAPS = np.stack([np.array([[0.7, 0.5, 0.5, 0.7]] * 3),
                         np.array([[0.7, 0.5, 0.5, 0.7], [0.5, 0.25, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5]])], 0)
# every kind clean_data distinguishes: the four classes, both neighbours, DontCare in both spellings, other case, other names
GT_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Bus'] * 3 + ['Van', 'Person_sitting', 'DontCare', 'dontcare', 'car', 'Truck', 'CYCLIST']
DT_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Bus'] * 2 + ['Truck', 'car']
DT_COUNTS = [0, 1, 63, 64, 65, 130]          # both sides of a wave, and a third chunk
GT_COUNTS = [0, 1, 7, 65]


def golden_annos():
    return [R.parse_label_text(str(t)) for t in GOLD['label_gt']], [R.parse_label_text(str(t)) for t in GOLD['label_dt']]


def _boxes(rng, n):
    """2-D boxes on a coarse grid: equal boxes, equal overlaps and every side of the three height limits (40, 25, 25) occur."""
    x1 = rng.choice([0.0, 50.0, 100.0, 400.0], n)
    y1 = rng.choice([0.0, 20.0], n)
    w = rng.choice([100.0, 150.0], n)
    h = rng.choice([20.0, 25.0, 30.0, 40.0, 41.0, 60.0, 60.0, 90.0, 90.0, 120.0], n)
    return np.stack([x1, y1, x1 + w, y1 + h], 1)


def _anno(rng, n, names, detection):
    a = {'name': np.array([names[k] for k in rng.integers(0, len(names), n)], dtype='<U14') if n else np.zeros(0, dtype='<U14'),
         'truncated': rng.choice([0.0, 0.0, 0.0, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6], n),
         'occluded': rng.choice([0.0, 0.0, 0.0, 1.0, 2.0, 3.0], n),
         'alpha': np.round(rng.uniform(-3, 3, n), 1), 'bbox': _boxes(rng, n),
         # l, h, w and a location grid of 2 m: rotated overlaps tie as well
         'dimensions': np.stack([rng.choice([3.5, 4.0], n), rng.choice([1.5, 1.6], n), rng.choice([1.6, 1.8], n)], 1),
         'location': np.stack([rng.integers(-5, 6, n) * 2.0, rng.choice([1.0, 1.2], n), rng.integers(5, 15, n) * 2.0], 1),
         'rotation_y': rng.choice([0.0, 0.3, 1.57], n)}
    if detection:
        a['truncated'], a['occluded'] = np.zeros(n), np.zeros(n)
        a['score'] = np.round(rng.uniform(0, 1, n), 1)                    # many ties
    else:
        a['score'] = np.zeros(n)
    return a


def stress_set(seed, images=14):
    """Random frames: tied scores, tied overlaps, empty images, all three ignore flags on both sides, DontCare boxes, and
    every per-image count of DT_COUNTS / GT_COUNTS at least once (the lists are walked with coprime strides)."""
    rng = np.random.default_rng(1000 + seed)
    gts, dts = [], []
    for m in range(images):
        G = GT_COUNTS[(m + seed) % 4] if m < 4 else int(rng.integers(0, 16))
        D = DT_COUNTS[(m * 5 + seed) % 6] if m < 6 else int(rng.integers(0, 24))
        g, d = _anno(rng, G, GT_NAMES, False), _anno(rng, D, DT_NAMES, True)
        for j in range(min(G, D)):                       # about half of the boxes are detected exactly, mostly under their name
            if rng.uniform() < 0.5:
                i = int(rng.integers(0, G))
                d['bbox'][j] = g['bbox'][i]
                if rng.uniform() < 0.8:
                    d['name'][j] = str(g['name'][i])[:10]
        gts.append(g)
        dts.append(d)
    return gts, dts


def random_overlaps(seed, gts, dts):
    """float32 [pairs] per rotated metric: rounded to 0.1 with many zeros (ties and values on the minimum overlaps)."""
    rng = np.random.default_rng(2000 + seed)
    n = sum(len(g['name']) * len(d['name']) for g, d in zip(gts, dts))
    return [(np.round(rng.uniform(0, 1, n), 1) * (rng.uniform(0, 1, n) < 0.6)).astype(np.float32) for _ in range(2)]


def crossing_set(images=40, per_image=26):
    """40 images x 26 cars with a detection exactly on every box and distinct-ish scores: the Car cells collect 1040 true
    positives, which crosses the sort's 1024 padding."""
    rng = np.random.default_rng(77)
    gts, dts = [], []
    for _ in range(images):
        n = per_image
        x1 = np.arange(n) * 70.0
        g = {'name': np.array(['Car'] * n), 'truncated': np.zeros(n), 'occluded': np.zeros(n), 'alpha': np.round(rng.uniform(-3, 3, n), 2),
             'bbox': np.stack([x1, np.zeros(n), x1 + 60.0, np.full(n, 50.0)], 1), 'dimensions': np.tile([4.0, 1.5, 1.8], (n, 1)),
             'location': np.stack([np.arange(n) * 6.0 - 70.0, np.full(n, 1.0), np.full(n, 30.0)], 1),
             'rotation_y': np.round(rng.uniform(-1, 1, n), 2), 'score': np.zeros(n)}
        d = {k: v.copy() for k, v in g.items()}
        d['alpha'] = g['alpha'] + np.round(rng.uniform(-0.5, 0.5, n), 2)
        d['score'] = np.round(rng.uniform(0.05, 1, n), 3)
        gts.append(g)
        dts.append(d)
    return gts, dts


def flat_overlaps(gts, dts, metric):
    """The oracle's float64 overlaps of a set as the float32 [pairs] array the host twin takes."""
    ov = [R.frame_overlaps(g, d, metric) for g, d in zip(gts, dts)]
    return np.concatenate([o.reshape(-1) for o in ov]).astype(np.float32) if ov else np.zeros(0, np.float32)


def yardstick_curves(gts, dts, classes, min_overlaps, flat_bev, flat_3d, compute_aos):
    """precision / recall / orientation [3, C, 3, 2, 41] and the threshold counts [3, C, 3, 2]: per cell ``clean_data`` over the
    set and one ``sgv3d_kitti_eval_curves`` call, the 2-D overlaps from ``image_box_overlap``, the rotated ones as given
    (float32, widened)."""
    lib = _lib.load()
    C, M = len(classes), len(gts)
    shape = (3, C, 3, 2, 41)
    prec, rec, ori, nthr = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape[:-1], np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    gt_num = np.array([len(g['name']) for g in gts], np.int32)
    dt_num = np.array([len(d['name']) for d in dts], np.int32)
    cat = lambda rows, w: np.ascontiguousarray(np.concatenate([np.asarray(r, np.float64).reshape(-1, w) for r in rows], 0))
    gtd = cat([np.concatenate([g['bbox'].reshape(-1, 4), g['alpha'].reshape(-1, 1)], 1) for g in gts], 5)
    dtd = cat([np.concatenate([d['bbox'].reshape(-1, 4), d['alpha'].reshape(-1, 1), d['score'].reshape(-1, 1)], 1) for d in dts], 6)
    ov2d = np.concatenate([image_box_overlap(d['bbox'], g['bbox']).reshape(-1) for g, d in zip(gts, dts)])
    flats = [np.ascontiguousarray(ov2d, np.float64), np.ascontiguousarray(flat_bev, np.float64), np.ascontiguousarray(flat_3d, np.float64)]
    for ci, cls in enumerate(classes):
        for diff in range(3):
            cl = [clean_data(g, d, cls, diff) for g, d in zip(gts, dts)]
            ig = np.ascontiguousarray(np.concatenate([c[1] for c in cl]), np.int64)
            idt = np.ascontiguousarray(np.concatenate([c[2] for c in cl]), np.int64)
            dc = np.ascontiguousarray(np.concatenate([c[3] for c in cl], 0), np.float64)
            dcn = np.array([len(c[3]) for c in cl], np.int32)
            for metric in range(3):
                for k in range(2):
                    n = ctypes.c_int(0)
                    p, r, o = prec[metric, ci, diff, k], rec[metric, ci, diff, k], ori[metric, ci, diff, k]
                    rc = lib.sgv3d_kitti_eval_curves(M, P(gt_num), P(dt_num), P(dcn), P(flats[metric]), P(gtd), P(dtd), P(ig), P(idt), P(dc),
                                                     metric, float(min_overlaps[k, metric, ci]), 1 if compute_aos and metric == 0 else 0,
                                                     sum(c[0] for c in cl), 1, P(p), P(r), P(o), ctypes.addressof(n))
                    assert rc == 0
                    nthr[metric, ci, diff, k] = n.value
    return prec, rec, ori, nthr


def assert_curves(got, want):
    """(precision, recall, orientation, num_thresholds): integers in and divisions out are bitwise, orientation sums cos."""
    np.testing.assert_array_equal(got[3], want[3])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_allclose(got[2], want[2], rtol=0, atol=1e-12, equal_nan=True)
