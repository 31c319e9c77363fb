"""GPU: the box decode with ``nms_type='rotate'`` (csrc/decode_rotate.hip through BEVHeightHead.get_bboxes and the C ABI)
against the float64 restatement tests/decode_rotate_ref.py (parity with mmdet3d unpinned, DESIGN.md "Box decode:
nms_type='rotate'").

The kernel decides ``IoU > nms_thr`` in float32, the reference in float64: the two can only be held to the same set of
boxes where no pair that the greedy walk actually decides (i kept, j > i still alive) has an IoU within the margin m of the
threshold.  m is 8 x the largest deviation of the HOST build of the kernel's geometry from the reference over the
overlapping candidate pairs of the inputs (decode_rotate_ref.margin, asserted <= 4e-5 in test_decode_rotate_cpu.py); the
condition is asserted on the reference before anything is compared.

m covers the float32 rounding of the GEOMETRY only.  In the get_bboxes and model tests the device's candidate boxes
themselves differ a little from numpy's (decode.hip is built with contraction, numpy rounds every operation: inside the
1e-3 box tolerance, in practice float32 ulps), which can move an IoU by a few 1e-6 more, about as much as m.  The decided
gaps of the inputs used here are 4.7e-5 and up, some ten times m, so the sets agree; a new seed whose smallest decided gap
comes close to m may pass the condition and still differ, and is then to be replaced, not the margin."""
import ctypes

import numpy as np
import pytest
import torch

import decode_rotate_ref as R
from oracle import decode_ref
from sgv3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _assert_decidable(decided, m, what):
    gaps = np.asarray([abs(iou - thr) for iou, thr in decided])
    print(f"{what}: {len(gaps)} decided pairs, smallest |IoU - nms_thr| = {gaps.min() if len(gaps) else float('nan'):.3g}, m = {m:.3g}")
    assert len(gaps) and gaps.min() >= m, (what, gaps.min(), m)


@pytest.mark.parametrize("H,W,B,max_num,seed", R.CASES)
def test_get_bboxes_rotate_matches_reference(H, W, B, max_num, seed):
    """The shapes and seeds of test_decode_gpu.py's circle test (max_num 600: the plain form with the bit matrix in the
    workspace); the post-NMS cap is active (83 survivors in most tasks)."""
    from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead
    hc = R.case_config(max_num)
    head = BEVHeightHead(**hc)
    buf, layout = R.fake_preds(B, H, W, seed)
    preds_cpu = tuple([{k: buf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)
    decided = []
    ref = R.get_bboxes_rotate(preds_cpu, hc['bbox_coder'], hc['test_cfg'], head.num_classes, decided=decided)
    m = R.margin()
    assert m <= 4e-5
    _assert_decidable(decided, m, f"{H}x{W} B{B} K{max_num}")
    dbuf = torch.from_numpy(buf).to(DEV)
    preds_gpu = tuple([{k: dbuf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)
    res = head.get_bboxes(preds_gpu, img_metas=[dict() for _ in range(B)])
    assert len(res) == B
    total = 0
    for i in range(B):
        boxes, scores, labels = res[i][0].tensor.cpu().numpy(), res[i][1].cpu().numpy(), res[i][2].cpu().numpy()
        rb, rs, rl = ref[i]
        print(f"sample {i}: {len(scores)} detections (reference {len(rs)})")
        assert boxes.shape == rb.shape and boxes.shape[1] == 9, (boxes.shape, rb.shape)
        assert np.array_equal(labels, rl)
        np.testing.assert_allclose(scores, rs, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(boxes, rb, rtol=1e-3, atol=1e-3)
        total += len(scores)
    assert total > 20


# ------------------------------------------------------------------------------------------------ the NMS stage alone
def _run_nms(boxes, scores, valid, nms_thr, score_threshold=0.0, pre_max_size=0, post_max_size=0, limit_range=None):
    """boxes [T, B, K, 9], scores / valid [T, B, K] (numpy) -> keep [T, B, K] from sgv3d_rotate_nms."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    T, B, K = scores.shape
    db = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(DEV)
    ds = torch.from_numpy(np.ascontiguousarray(scores, np.float32)).to(DEV)
    dv = torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).to(DEV)
    keep = torch.full((T, B, K), 7, dtype=torch.uint8, device=DEV)
    nws = lib.sgv3d_rotate_nms_workspace_bytes(B, T, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    lim = (ctypes.c_float * 6)(*limit_range) if limit_range is not None else None
    rc = lib.sgv3d_rotate_nms(B, T, K, db.data_ptr(), ds.data_ptr(), dv.data_ptr(), float(score_threshold),
                              (ctypes.c_float * T)(*nms_thr), int(pre_max_size), int(post_max_size), lim, ws.data_ptr(), nws,
                              keep.data_ptr(), _lib.stream_handle(torch.device(DEV)))
    _lib.check(rc, "sgv3d_rotate_nms")
    torch.cuda.synchronize()
    return keep.cpu().numpy()


def _ref_nms(boxes, scores, valid, nms_thr, score_threshold=0.0, pre_max_size=0, post_max_size=0, limit_range=None, decided=None):
    T, B, K = scores.shape
    keep = np.zeros((T, B, K), np.uint8)
    for t in range(T):
        for b in range(B):
            idx = np.nonzero(valid[t, b])[0]
            pairs = []
            k = R.nms_rotate(boxes[t, b][idx], scores[t, b][idx], nms_thr[t], score_threshold, pre_max_size, post_max_size,
                             limit_range, pairs)
            keep[t, b, idx[k]] = 1
            if decided is not None:
                decided.extend((iou, nms_thr[t]) for _, _, iou in pairs)
    return keep


def _hand(rows, K=None):
    """rows of (x, y, z, d0, d1, yaw), best first -> boxes [1, 1, K, 9], scores [1, 1, K], valid [1, 1, K] (padded invalid)."""
    n = len(rows)
    K = K or n
    boxes = np.zeros((1, 1, K, 9), np.float32)
    for i, (x, y, z, d0, d1, yaw) in enumerate(rows):
        boxes[0, 0, i, :7] = [x, y, z, d0, d1, 1.5, yaw]
    scores = np.zeros((1, 1, K), np.float32)
    scores[0, 0, :n] = np.linspace(0.9, 0.3, n, dtype=np.float32) if n > 1 else 0.9
    valid = np.zeros((1, 1, K), np.uint8)
    valid[0, 0, :n] = 1
    return boxes, scores, valid


def _both(args, **kw):
    got, want = _run_nms(*args, [0.2], **kw), _ref_nms(*args, [0.2], **kw)
    assert np.array_equal(got, want), (got[0, 0], want[0, 0])
    return list(np.nonzero(got[0, 0])[0])


def test_rotate_nms_parallel_long_vehicles_both_survive():
    """Two 12 m x 2.5 m boxes side by side, 3 m apart: disjoint rectangles, both kept.  Circle NMS with the truck task's
    radius (min_radius 12, compared with the SQUARED distance 9) drops the second."""
    args = _hand([(30, 0, 0, 12, 2.5, 0.02), (30, 3, 0, 12, 2.5, 0.02)])
    assert _both(args) == [0, 1]
    dets = np.concatenate([args[0][0, 0, :, :2], args[1][0, 0, :, None]], 1)
    assert list(decode_ref.circle_nms(dets, 12, 83)) == [0]


def test_rotate_nms_crossed_boxes():
    # a 6 x 1 box crossed by the same box turned a quarter: IoU = 1 / 11 < 0.2, both stay; a 2 x 1 pair crossed: 1 / 3 > 0.2
    assert _both(_hand([(10, 5, 0, 6, 1, 0.0), (10, 5, 0, 6, 1, np.pi / 2)])) == [0, 1]
    assert _both(_hand([(10, 5, 0, 2, 1, 0.0), (10, 5, 0, 2, 1, np.pi / 2)])) == [0]


def test_rotate_nms_caps_thresholds_and_ranges():
    rows = [(0, 0, 0, 4, 2, 0), (0.2, 0, 0, 4, 2, 0), (10, 0, 0, 4, 2, 0), (10, 0.1, 0, 4, 2, 0.05), (20, 0, 0, 4, 2, 0)]
    args = _hand(rows, K=8)
    assert _both(args) == [0, 2, 4]
    assert _both(args, pre_max_size=2) == [0]                      # cuts before the walk
    assert _both(args, pre_max_size=4) == [0, 2]
    assert _both(args, post_max_size=1) == [0]                     # cuts after it
    assert _both(args, post_max_size=2) == [0, 2]
    # scores are linspace(0.9, 0.3, 5) = .9 .75 .6 .45 .3: a test threshold above the coder's, inclusive
    assert _both(args, score_threshold=float(args[1][0, 0, 2])) == [0, 2]
    assert _both(args, score_threshold=0.61) == [0]
    # the best candidate is not valid for the coder: it takes no part, so the second is kept
    b, s, v = _hand(rows, K=8)
    v[0, 0, 0] = 0
    assert _both((b, s, v)) == [1, 2, 4]
    # a limit range narrower than the coder's: 0 lies outside, has suppressed 1 and used a post_max_size slot
    out = _hand([(-1, 0, 0, 4, 2, 0), (0.5, 0, 0, 4, 2, 0), (10, 0, 0, 4, 2, 0), (0, -5, 5, 4, 2, 0)])
    lim = [0, -5, -5, 50, 5, 5]
    assert _both(out, limit_range=lim) == [2, 3]                   # (3 sits on the inclusive bounds)
    assert _both(out) == [0, 2, 3]
    assert _both(out, limit_range=lim, post_max_size=1) == []
    assert _both(out, limit_range=lim, post_max_size=2) == [2]


def test_rotate_nms_degenerate_and_non_finite_boxes_are_inert():
    rows = [(0, 0, 0, 4, 0, 0), (0, 0, 0, 4, 2, 0), (0, 0, 0, 4, 2, np.nan), (0.1, 0, 0, 4, 2, 0), (np.inf, 0, 0, 4, 2, 0),
            (0, 0, 0, -4, 2, 0), (0, np.nan, 0, 4, 2, 0), (0, 0.1, 0, np.inf, 2, 0)]
    assert _both(_hand(rows)) == [0, 1, 2, 4, 5, 6, 7]
    # with a range, a non-finite centre fails the range test like any centre outside it
    assert _both(_hand(rows), limit_range=[-50, -50, -5, 50, 50, 5]) == [0, 1, 2, 5, 7]


def test_rotate_nms_no_candidates():
    b, s, v = _hand([(0, 0, 0, 4, 2, 0)], K=500)
    v[:] = 0
    assert _both((b, s, v)) == []
    assert _both(_hand([(0, 0, 0, 4, 2, 0)], K=500), score_threshold=0.95) == []


def _crowd(T, B, K, seed, n_valid=None):
    """K boxes per (task, sample) crowded into 40 m x 40 m (~20 neighbours each), descending scores."""
    g = np.random.default_rng(seed)
    boxes = np.zeros((T, B, K, 9), np.float32)
    boxes[..., 0] = g.uniform(40, 80, (T, B, K))
    boxes[..., 1] = g.uniform(-20, 20, (T, B, K))
    boxes[..., 2] = g.uniform(-2, 0, (T, B, K))
    boxes[..., 3] = g.uniform(3.5, 5.0, (T, B, K))
    boxes[..., 4] = g.uniform(1.6, 2.2, (T, B, K))
    boxes[..., 5] = 1.5
    boxes[..., 6] = g.uniform(-np.pi, np.pi, (T, B, K))
    scores = -np.sort(-g.uniform(0.1, 1.0, (T, B, K)).astype(np.float32), axis=-1)
    valid = np.ones((T, B, K), np.uint8)
    if n_valid is not None:
        valid[:] = 0
        for t in range(T):
            for b in range(B):
                valid[t, b, np.sort(g.choice(K, n_valid, replace=False))] = 1
    return boxes, scores, valid


@pytest.mark.parametrize("K,n_valid,post,pre,sthr", [(500, None, 83, 1000, 0.3), (512, None, 0, 0, 0.0), (500, 300, 0, 250, 0.0),
                                                     (600, None, 83, 1000, 0.3), (600, 577, 0, 0, 0.0), (1024, None, 0, 1000, 0.0)])
def test_rotate_nms_crowds(K, n_valid, post, pre, sthr):
    """n = K candidates (every one valid and above the threshold), gaps in the valid mask, a pre_max_size below the count, both forms (K <= 512: bit matrix in LDS; K = 600 and 1024:
    the plain form), two tasks with different thresholds, two samples, with and without the caps.  The margin is taken on
    these very boxes by the rule of decode_rotate_ref.margin; a crowd with a decided pair inside it is not usable (another
    seed would be, and would be noted here: none was needed)."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    T, B = 2, 2
    boxes, scores, valid = _crowd(T, B, K, seed=K + (n_valid or 0), n_valid=n_valid)
    thr = [0.2, 0.45]
    dev = 0.0
    for t in range(T):
        for b in range(B):
            b5 = boxes[t, b][:, R.BEV]
            i, j = R.overlapping_pairs(b5)
            want = np.asarray([R.bev_iou(b5[p], b5[q]) for p, q in zip(i, j)])
            dev = max(dev, float(np.abs(R.host_iou(lib, b5[i], b5[j]) - want).max()))
    m = 8 * dev
    assert 0 < m <= 4e-5, m
    decided = []
    want = _ref_nms(boxes, scores, valid, thr, sthr, pre, post, None, decided)
    _assert_decidable(decided, m, f"crowd K{K}")
    got = _run_nms(boxes, scores, valid, thr, sthr, pre, post, None)
    print("kept per (task, sample):", got.sum(-1).tolist())
    assert np.array_equal(got, want), np.nonzero(got != want)
    assert 0 < got.sum() < valid.sum()


# ------------------------------------------------------------------------------------------------ both entries
def test_one_call_entry_is_candidate_stage_plus_rotate_nms():
    """sgv3d_centerpoint_decode_tasks_rotate gives the bytes of the candidate stage (through the circle entry, which shares it)
    followed by sgv3d_rotate_nms."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    hc = R.case_config(500)
    coder, tcfg = hc['bbox_coder'], hc['test_cfg']
    B, H, W, K = 2, 128, 128, 500
    buf, layout = R.fake_preds(B, H, W, seed=77)
    dbuf = torch.from_numpy(buf).to(DEV)
    T = len(layout)
    ptrs = {k: (ctypes.c_void_p * T)(*[dbuf[:, d[k][0]:].data_ptr() for d in layout]) for k in layout[0]}
    cats = (ctypes.c_int32 * T)(*[d['heatmap'][1] for d in layout])
    max_cat = max(cats)
    rng_c = (ctypes.c_float * 6)(*[float(v) for v in coder['post_center_range']])
    lim_c = (ctypes.c_float * 6)(*[float(v) for v in tcfg['post_center_limit_range']])
    thr_c = (ctypes.c_float * T)(*[float(tcfg['nms_thr'])] * T)
    stream = _lib.stream_handle(torch.device(DEV))

    def outputs():
        return dict(boxes=torch.zeros(T, B, K, 9, device=DEV), scores=torch.zeros(T, B, K, device=DEV),
                    labels=torch.zeros(T, B, K, dtype=torch.int32, device=DEV), valid=torch.zeros(T, B, K, dtype=torch.uint8, device=DEV),
                    keep=torch.zeros(T, B, K, dtype=torch.uint8, device=DEV))

    front = (B, T, cats, H, W, K, ptrs['heatmap'], ptrs['reg'], ptrs['height'], ptrs['dim'], ptrs['rot'], ptrs['vel'],
             int(dbuf.stride(0)), float(coder['out_size_factor']), float(coder['voxel_size'][0]), float(coder['voxel_size'][1]),
             float(coder['pc_range'][0]), float(coder['pc_range'][1]), float(coder['score_threshold']), rng_c, 1)
    one = outputs()
    nws = lib.sgv3d_centerpoint_decode_tasks_rotate_workspace_bytes(B, T, max_cat, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc = lib.sgv3d_centerpoint_decode_tasks_rotate(*front, float(tcfg['score_threshold']), thr_c, int(tcfg['pre_max_size']),
                                                   int(tcfg['post_max_size']), lim_c, ws.data_ptr(), nws,
                                                   *[one[k].data_ptr() for k in ('boxes', 'scores', 'labels', 'valid', 'keep')], stream)
    _lib.check(rc, "sgv3d_centerpoint_decode_tasks_rotate")
    two = outputs()
    nws2 = lib.sgv3d_centerpoint_decode_tasks_workspace_bytes(B, T, max_cat, K)
    ws2 = torch.empty(nws2, dtype=torch.uint8, device=DEV)
    radii = (ctypes.c_float * T)(*[float(v) for v in tcfg['min_radius']])
    rc = lib.sgv3d_centerpoint_decode_tasks(*front, radii, int(tcfg['post_max_size']), ws2.data_ptr(), nws2,
                                            *[two[k].data_ptr() for k in ('boxes', 'scores', 'labels', 'valid', 'keep')], stream)
    _lib.check(rc, "sgv3d_centerpoint_decode_tasks")
    circle_keep = two['keep'].clone()
    nws3 = lib.sgv3d_rotate_nms_workspace_bytes(B, T, K)
    ws3 = torch.empty(nws3, dtype=torch.uint8, device=DEV)
    rc = lib.sgv3d_rotate_nms(B, T, K, two['boxes'].data_ptr(), two['scores'].data_ptr(), two['valid'].data_ptr(),
                              float(tcfg['score_threshold']), thr_c, int(tcfg['pre_max_size']), int(tcfg['post_max_size']), lim_c,
                              ws3.data_ptr(), nws3, two['keep'].data_ptr(), stream)
    _lib.check(rc, "sgv3d_rotate_nms")
    torch.cuda.synchronize()
    for k in one:
        assert torch.equal(one[k], two[k]), k
    assert 0 < int(one['keep'].sum()) and not torch.equal(one['keep'], circle_keep)


# ------------------------------------------------------------------------------------------------ the model
def _small_model(seed=0):
    from sgv3d_amd.models.bev_height import BEVHeight
    bc, hc = S.small_conf(depth=18)
    torch.manual_seed(seed)
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 1)
    with torch.no_grad():                                    # make some heat rise above the 0.1 threshold
        for th in m.head.task_heads:
            th.heatmap[1].bias.fill_(-1.0)
            th.heatmap[1].weight.mul_(3.0)
    m = m.to(DEV)
    imgs, mats = S.make_images(2, bc['final_dim'], device=DEV, seed=4), S.make_mats(2, device=DEV, scale=128 / 864)
    return m, hc, imgs, mats


def _rows(res):
    return [(r[0].tensor.clone(), r[1].clone(), r[2].clone()) for r in res]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_full_model_rotate_decode_matches_reference():
    """Forward + get_bboxes of the small config (as test_decode_gpu.py::test_full_model_decode_runs, seed 0) with the rotate
    config, against the reference on the HIP maps; the margin condition is checked on those maps first."""
    m, hc, imgs, mats = _small_model()
    m.head.test_cfg = dict(m.head.test_cfg, nms_type='rotate')
    m.graph_forward = False
    with torch.no_grad():
        preds = m(imgs, mats)
        res = m.get_bboxes(preds, [dict(), dict()])
    preds_cpu = tuple([{k: v.cpu().numpy() for k, v in p[0].items()}] for p in preds)
    decided = []
    ref = R.get_bboxes_rotate(preds_cpu, hc['bbox_coder'], m.head.test_cfg, m.head.num_classes, decided=decided)
    _assert_decidable(decided, R.margin(), "small model, seed 0")
    for i in range(2):
        print(f"sample {i}: {len(res[i][1])} detections (reference {len(ref[i][1])})")
        assert res[i][0].tensor.shape == ref[i][0].shape
        np.testing.assert_allclose(res[i][0].tensor.cpu().numpy(), ref[i][0], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(res[i][1].cpu().numpy(), ref[i][1], rtol=1e-5, atol=1e-6)
        assert np.array_equal(res[i][2].cpu().numpy(), ref[i][2])


def test_graphed_rotate_decode_and_switching_nms_type():
    """The graphed forward's pre-decoded buffer holds what an eager decode_device of the same maps gives, byte for byte (counts,
    and every row below them; the rows above are never written); and one model instance switched between 'circle' and
    'rotate' never answers with the other type's decode -- neither from a recorded graph nor from the buffer a forward left
    behind before the switch."""
    m, hc, imgs, mats = _small_model()
    head = m.head
    circle_cfg, rotate_cfg = dict(head.test_cfg, nms_type='circle'), dict(head.test_cfg, nms_type='rotate')
    metas = [dict(), dict()]

    def eager(cfg):
        head.test_cfg = cfg
        m.graph_forward = False
        with torch.no_grad():
            out = _rows(m.get_bboxes(m(imgs, mats), metas))
        m.graph_forward = True
        return out

    want_circle, want_rotate = eager(circle_cfg), eager(rotate_cfg)
    assert not _same(want_circle, want_rotate), "the two NMS types agree on these maps: the test would show nothing"
    assert not m._graphs
    with torch.no_grad():
        head.test_cfg = rotate_cfg
        m(imgs, mats)                                        # first sight: eager
        preds = m(imgs, mats)                                # capture + replay
        (entry,) = m._graphs.values()
        assert entry[1] and entry[1].replays == 1 and m._decoded is not None
        packed = m._decoded[0]
        again = head.decode_device(preds)
        B = 2
        gb, gs, gl, gc = head.decode_views(packed, B)
        eb, es, el, ec = head.decode_views(again, B)
        assert torch.equal(gc, ec)
        for i, n in enumerate(gc.tolist()):
            assert n > 0 and torch.equal(gb[i, :n], eb[i, :n]) and torch.equal(gs[i, :n], es[i, :n]) and torch.equal(gl[i, :n], el[i, :n])
        assert _same(_rows(m.get_bboxes(preds, metas)), want_rotate)
        # the buffer a rotate forward left behind is not served after the switch to circle ...
        preds = m(imgs, mats)
        assert m._decoded is not None
        head.test_cfg = circle_cfg
        assert _same(_rows(m.get_bboxes(preds, metas)), want_circle)
        # ... nor is the rotate graph: circle gets a graph of its own
        m(imgs, mats)
        assert len(m._graphs) == 2
        assert _same(_rows(m.get_bboxes(m(imgs, mats), metas)), want_circle)
        assert all(e[1] for e in m._graphs.values())
        # and back: the recorded rotate graph answers rotate
        head.test_cfg = rotate_cfg
        assert _same(_rows(m.get_bboxes(m(imgs, mats), metas)), want_rotate)
        assert len(m._graphs) == 2
        head.test_cfg = dict(head.test_cfg, nms_type='max_pool')
        with pytest.raises(AssertionError, match="nms_type"):
            head.decode_device(preds)
