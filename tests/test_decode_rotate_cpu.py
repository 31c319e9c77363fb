"""CPU: the rotated-IoU NMS of the box decode (csrc/decode_rotate.hip, ``nms_type='rotate'``) without a GPU -- the float64
reference (tests/decode_rotate_ref.py) on cases with analytic answers, the host build of the kernel's float32 geometry
(``sgv3d_rotated_bev_iou_host``) against it, the C ABI's argument checks, and the reference NMS on hand cases.  Parity with
mmdet3d is unpinned (DESIGN.md "Box decode: nms_type='rotate'")."""
import ctypes
import math

import numpy as np
import pytest

import decode_rotate_ref as R

# (a5, b5, IoU) with answers worked out by hand
SQ2 = math.sqrt(2.0)
ANALYTIC = [
    ("identical", [3, 4, 4, 2, 0.7], [3, 4, 4, 2, 0.7], 1.0),
    ("axis-aligned partial overlap", [0, 0, 2, 2, 0], [1, 1, 2, 2, 0], 1.0 / 7.0),
    ("unit square against itself turned 45 degrees", [0, 0, 1, 1, 0], [0, 0, 1, 1, math.pi / 4],
     2 * (SQ2 - 1) / (2 - 2 * (SQ2 - 1))),
    ("disjoint", [0, 0, 2, 2, 0], [5, 0, 2, 2, 0.3], 0.0),
    ("touching along an edge", [0, 0, 2, 2, 0], [2, 0, 2, 2, 0], 0.0),
    ("one inside the other", [10, -5, 4, 4, 0.3], [10, -5, 2, 1, 1.1], 2.0 / 16.0),
    ("quarter turn of a 4 x 2 box", [0, 0, 4, 2, 0], [0, 0, 4, 2, math.pi / 2], 4.0 / 12.0),
]


@pytest.fixture(scope="module")
def lib():
    from sgv3d_amd import _lib
    return _lib.load()


def test_reference_analytic_cases():
    assert abs(R.intersection([0, 0, 1, 1, 0], [0, 0, 1, 1, math.pi / 4]) - 2 * (SQ2 - 1)) < 1e-12
    for name, a, b, want in ANALYTIC:
        assert abs(R.bev_iou(a, b) - want) < 1e-12, name
        assert abs(R.bev_iou(b, a) - want) < 1e-12, name


def test_reference_convention_is_clockwise():
    """A 4 x 1 box at yaw 0.5 against a level one up and to the right: under this build's convention (a corner offset
    (ox, oy) -> (ox cos + oy sin, -ox sin + oy cos)) positive yaw turns the long axis towards -y, away from the second box.
    The counter-clockwise convention turns it towards the second box and gives a different IoU."""
    a, b = [0, 0, 4, 1, 0.5], [0.5, 0.8, 4, 1, 0.0]
    cw = R.bev_iou(a, b)
    ccw = R.bev_iou([0, 0, 4, 1, -0.5], b)                # the other convention = the mirrored angle
    c = R.corners(a)
    # the (+d0/2, +d1/2) corner: (2 cos .5 + .5 sin .5, -2 sin .5 + .5 cos .5)
    np.testing.assert_allclose(c[2], [2 * math.cos(.5) + .5 * math.sin(.5), -2 * math.sin(.5) + .5 * math.cos(.5)], atol=1e-12)
    assert abs(cw - ccw) > 1e-2, (cw, ccw)                # (0.156 against 0.205: far beyond any rounding)
    assert cw < ccw


def test_host_geometry_on_analytic_cases(lib):
    a = [c[1] for c in ANALYTIC] + [[0, 0, 4, 1, 0.5]]
    b = [c[2] for c in ANALYTIC] + [[0.5, 0.8, 4, 1, 0.0]]
    want = [c[3] for c in ANALYTIC] + [R.bev_iou(a[-1], b[-1])]
    got = R.host_iou(lib, a, b)
    print("host - analytic:", got - np.asarray(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-7)
    # far from the origin the answer is the same: the arithmetic is relative to the first box's centre
    far = np.asarray([120.0, -60.0, 0, 0, 0])
    np.testing.assert_allclose(R.host_iou(lib, np.asarray(a) + far, np.asarray(b) + far), want, rtol=0, atol=5e-7)


def test_host_geometry_degenerate_boxes_are_inert(lib):
    ok = [1, 1, 2, 2, 0.1]
    bad = [[np.nan, 1, 2, 2, 0.1], [1, np.inf, 2, 2, 0.1], [1, 1, 0, 2, 0.1], [1, 1, 2, -1, 0.1], [1, 1, np.inf, 2, 0.1],
           [1, 1, 2, 2, np.nan], [1, 1, 2, np.nan, 0.1]]
    for b in bad:
        assert R.bev_iou(ok, b) == 0.0 and R.bev_iou(b, ok) == 0.0 and R.bev_iou(b, b) == 0.0
    assert (R.host_iou(lib, [ok] * len(bad), bad) == 0).all() and (R.host_iou(lib, bad, [ok] * len(bad)) == 0).all()
    assert (R.host_iou(lib, bad, bad) == 0).all()


def test_host_geometry_on_candidate_pairs_and_margin(lib):
    """Every overlapping candidate pair of the GPU test inputs: the deviation of the float32 host build from the float64
    reference, times 8, is the margin m of tests/test_decode_rotate_gpu.py.  It comes from the reference, not from a
    device.  Centre-relative float32 is expected around 2e-6; above 4e-5 the arithmetic would be badly conditioned (the
    smallest gap between a decided pair's IoU and nms_thr in those inputs is 4.7e-5)."""
    m = R.margin()
    for case in R.CASES:
        dev, count = R.host_deviation(case)
        assert count > 1000, (case, count)
    assert 0 < m <= 4e-5, m


def test_abi_argument_validation(lib):
    thr = (ctypes.c_float * 16)(*[0.2] * 16)
    p = ctypes.c_void_p(256)                         # never dereferenced: every call below fails its checks first
    ws = lib.sgv3d_rotate_nms_workspace_bytes(1, 1, 600)

    def nms(batch=1, tasks=1, K=600, boxes=p, scores=p, valid=p, thr_=thr, wsp=p, nbytes=ws, keep=p):
        return lib.sgv3d_rotate_nms(batch, tasks, K, boxes, scores, valid, 0.1, thr_, 1000, 83, None, wsp, nbytes, keep, None)

    for kw, word in ((dict(batch=0), b"non-positive"), (dict(tasks=0), b"non-positive"), (dict(K=0), b"non-positive"),
                     (dict(tasks=17), b"16 tasks"), (dict(K=1025), b"exceeds"), (dict(boxes=None), b"null"),
                     (dict(scores=None), b"null"), (dict(valid=None), b"null"), (dict(thr_=None), b"null"), (dict(wsp=None), b"null"),
                     (dict(keep=None), b"null"), (dict(nbytes=ws - 1), b"workspace"), (dict(wsp=ctypes.c_void_p(260)), b"aligned")):
        assert nms(**kw) == -1, kw
        assert word in lib.sgv3d_last_error(), (kw, lib.sgv3d_last_error())

    neg = (ctypes.c_float * 16)(0.2, -0.1)
    assert nms(tasks=2, thr_=neg) == -1 and b"nms_thr[1]" in lib.sgv3d_last_error()
    cats = (ctypes.c_int32 * 17)(*[1] * 17)
    ptrs = (ctypes.c_void_p * 17)(*[256] * 17)
    wsd = lib.sgv3d_centerpoint_decode_tasks_rotate_workspace_bytes(1, 2, 1, 500)

    def decode(batch=1, tasks=2, h=64, K=500, cats_=cats, heat=ptrs, thr_=thr, wsp=p, nbytes=wsd, boxes=p):
        return lib.sgv3d_centerpoint_decode_tasks_rotate(batch, tasks, cats_, h, 64, K, heat, ptrs, ptrs, ptrs, ptrs, None, 4096, 4.0,
                                                         0.1, 0.1, 0.0, -51.2, 0.1, None, 1, 0.1, thr_, 1000, 83, None, wsp, nbytes,
                                                         boxes, p, p, p, p, None)

    for kw, word in ((dict(batch=0), b"non-positive"), (dict(tasks=0), b"non-positive"), (dict(h=0), b"non-positive"),
                     (dict(K=0), b"non-positive"), (dict(tasks=17), b"16 tasks"), (dict(cats_=None), b"null"),
                     (dict(thr_=None), b"null"), (dict(wsp=None), b"null"), (dict(nbytes=wsd - 1), b"workspace"),
                     (dict(heat=None), b"null"), (dict(boxes=None), b"null"), (dict(K=1025), b"too large")):
        assert decode(**kw) == -1, kw
        assert word in lib.sgv3d_last_error(), (kw, lib.sgv3d_last_error())
    assert decode(thr_=neg) == -1 and b"nms_thr[1]" in lib.sgv3d_last_error()
    assert lib.sgv3d_rotated_bev_iou_host(-1, None, None, None) == -1
    assert lib.sgv3d_rotated_bev_iou_host(2, None, None, None) == -1 and b"null" in lib.sgv3d_last_error()
    assert lib.sgv3d_rotated_bev_iou_host(0, None, None, None) == 0


def test_workspace_bytes(lib):
    f = lib.sgv3d_rotate_nms_workspace_bytes
    assert 0 < f(2, 6, 100) <= f(2, 6, 512) < f(2, 6, 513) < f(2, 6, 600) < f(2, 6, 1024)
    assert f(2, 6, 600) >= 2 * 6 * 600 * (1024 // 64) * 8            # the plain form's bit matrix
    assert f(2, 6, 600) < f(4, 6, 600) and f(2, 6, 600) < f(2, 12, 600)
    assert f(0, 6, 500) == 0 and f(2, 0, 500) == 0 and f(2, 6, 0) == 0 and f(2, 6, 1025) == 0 and f(-1, 6, 500) == 0
    g = lib.sgv3d_centerpoint_decode_tasks_rotate_workspace_bytes
    assert g(2, 6, 2, 600) >= lib.sgv3d_centerpoint_decode_tasks_workspace_bytes(2, 6, 2, 600) + f(2, 6, 600)
    assert g(2, 6, 0, 600) == 0 and g(2, 6, 2, 1025) == 0


# ---------------------------------------------------------------------------------------- the reference NMS on hand cases
def _boxes(rows):
    """rows of (x, y, z, d0, d1, yaw) -> [n, 9]"""
    out = np.zeros((len(rows), 9), np.float32)
    for i, (x, y, z, d0, d1, yaw) in enumerate(rows):
        out[i, :7] = [x, y, z, d0, d1, 1.5, yaw]
    return out


def test_nms_rotate_basic_and_caps():
    # 0 and 1 overlap heavily, 2 is apart, 3 overlaps 2 heavily, 4 is apart
    b = _boxes([(0, 0, 0, 4, 2, 0), (0.2, 0, 0, 4, 2, 0), (10, 0, 0, 4, 2, 0), (10, 0.1, 0, 4, 2, 0.05), (20, 0, 0, 4, 2, 0)])
    s = np.asarray([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    assert list(R.nms_rotate(b, s, 0.2)) == [0, 2, 4]
    # pre_max_size cuts BEFORE the walk: candidate 2 never takes part, so 3 is not looked at either
    assert list(R.nms_rotate(b, s, 0.2, pre_max_size=2)) == [0]
    assert list(R.nms_rotate(b, s, 0.2, pre_max_size=4)) == [0, 2]
    # post_max_size cuts AFTER it
    assert list(R.nms_rotate(b, s, 0.2, post_max_size=1)) == [0]
    assert list(R.nms_rotate(b, s, 0.2, post_max_size=2)) == [0, 2]
    assert list(R.nms_rotate(b, s, 0.2, pre_max_size=0, post_max_size=None)) == [0, 2, 4]
    # strict comparison: IoU(0, 1) = 3.8 / 4.2 / ... ; a threshold at or above it keeps both
    iou01 = R.bev_iou(b[0, R.BEV], b[1, R.BEV])
    assert list(R.nms_rotate(b[:2], s[:2], iou01)) == [0, 1] and list(R.nms_rotate(b[:2], s[:2], iou01 - 1e-9)) == [0]


def test_nms_rotate_score_threshold_is_inclusive():
    b = _boxes([(0, 0, 0, 4, 2, 0), (10, 0, 0, 4, 2, 0), (20, 0, 0, 4, 2, 0)])
    s = np.asarray([0.9, 0.5, 0.3], np.float32)
    assert list(R.nms_rotate(b, s, 0.2, score_threshold=0.5)) == [0, 1]          # >=: the coder's own test is >
    assert list(R.nms_rotate(b, s, 0.2, score_threshold=float(np.nextafter(np.float32(0.5), np.float32(1))))) == [0]
    assert list(R.nms_rotate(b, s, 0.2, score_threshold=0.0)) == [0, 1, 2]


def test_nms_rotate_outside_box_suppresses_then_leaves():
    # 0 lies outside the limit range and overlaps 1, which lies inside; 2 is inside and apart
    b = _boxes([(-1, 0, 0, 4, 2, 0), (0.5, 0, 0, 4, 2, 0), (10, 0, 0, 4, 2, 0)])
    s = np.asarray([0.9, 0.8, 0.7], np.float32)
    lim = [0, -5, -5, 50, 5, 5]
    assert list(R.nms_rotate(b, s, 0.2, limit_range=lim)) == [2]
    assert list(R.nms_rotate(b, s, 0.2, limit_range=[])) == [0, 2]
    # ... and it has used a post_max_size slot
    assert list(R.nms_rotate(b, s, 0.2, post_max_size=1, limit_range=lim)) == []
    # inclusive bounds, on the centre z before the merge lowers it
    edge = _boxes([(0, -5, 5, 4, 2, 0)])
    assert list(R.nms_rotate(edge, s[:1], 0.2, limit_range=lim)) == [0]


def test_nms_rotate_degenerate_box_is_inert():
    b = _boxes([(0, 0, 0, 4, 0, 0), (0, 0, 0, 4, 2, 0), (0, 0, 0, 4, 2, np.nan), (0.1, 0, 0, 4, 2, 0)])
    s = np.asarray([0.9, 0.8, 0.7, 0.6], np.float32)
    # 0 (zero width) and 2 (NaN yaw) neither suppress nor are suppressed; 1 suppresses 3
    assert list(R.nms_rotate(b, s, 0.2)) == [0, 1, 2]
    assert list(R.nms_rotate(b, s, 0.0)) == [0, 1, 2]
