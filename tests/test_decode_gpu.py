"""GPU: box decode + circle NMS (csrc/decode.hip through BEVHeightHead.get_bboxes) against the numpy
restatement of mmdet3d's CenterHead.get_bboxes (oracle/decode_ref.py; parity unpinned)."""
import functools

import numpy as np
import pytest
import torch

import decode_circle_ref as C
from oracle import decode_ref
from sgv3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fake_preds(B, H, W, seed, n_obj=40):
    """Head-like maps: low background heat with Gaussian blobs (so that > max_num pixels compete)."""
    g = np.random.default_rng(seed)
    names = [('reg', 2), ('height', 1), ('dim', 3), ('rot', 2), ('vel', 2)]
    ncls = [1, 2, 2, 1, 2, 2]
    buf = g.standard_normal((B, 70, H, W)).astype(np.float32) * 0.3
    preds, off = [], 0
    yy, xx = np.mgrid[0:H, 0:W]
    for t, nc in enumerate(ncls):
        d = {}
        for n, c in names:
            d[n] = (off, c)
            off += c
        d['heatmap'] = (off, nc)
        hm = buf[:, off:off + nc]
        hm[:] = hm * 0.5 - 4.0
        for b in range(B):
            for _ in range(n_obj):
                c, y, x = g.integers(nc), g.integers(H), g.integers(W)
                hm[b, c] += 6.5 * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * g.uniform(1.0, 6.0)))
        off += nc
        preds.append(d)
    return buf, preds


@pytest.mark.parametrize("H,W,B,max_num", [(256, 256, 2, 500), (64, 96, 1, 500), (128, 128, 2, 600), (512, 512, 1, 500)])
def test_get_bboxes_matches_oracle(H, W, B, max_num):
    """(max_num 600: the plain circle-NMS kernel, K > 512; 512 x 512: the top-k form without the cached keys)"""
    from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead
    _, hc = S.r50_256_conf()
    hc['bbox_coder'] = dict(hc['bbox_coder'], max_num=max_num)
    head = BEVHeightHead(**hc)
    buf, layout = _fake_preds(B, H, W, seed=H)
    dbuf = torch.from_numpy(buf).to(DEV)
    preds_gpu = tuple([{k: dbuf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)
    preds_cpu = tuple([{k: buf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)
    res = head.get_bboxes(preds_gpu, img_metas=[dict() for _ in range(B)])
    ref = decode_ref.get_bboxes(preds_cpu, hc['bbox_coder'], hc['test_cfg'], head.num_classes)
    assert len(res) == B
    total = 0
    for i in range(B):
        boxes, scores, labels = res[i][0].tensor.cpu().numpy(), res[i][1].cpu().numpy(), res[i][2].cpu().numpy()
        rb, rs, rl = ref[i]
        assert boxes.shape == rb.shape and boxes.shape[1] == 9, (boxes.shape, rb.shape)
        assert np.array_equal(labels, rl)
        np.testing.assert_allclose(scores, rs, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(boxes, rb, rtol=1e-3, atol=1e-3)      # north_star: box regressions within 1e-3
        # centres round once per operation as the oracle's do (decode.hip is built without contraction); vel is copied through
        assert np.array_equal(boxes[:, [0, 1, 7, 8]], rb[:, [0, 1, 7, 8]])
        total += len(scores)
        # per task at most post_max_size survive, everything above the score threshold
        assert (scores > hc['bbox_coder']['score_threshold']).all()
    assert total > 20


def test_circle_nms_known_answer():
    """Three collinear centres 1 m apart, radius^2 = 1.5: the middle (2nd best) one is suppressed by the best."""
    dets = np.array([[0, 0, 0.9], [1, 0, 0.8], [2, 0, 0.7], [10, 10, 0.95]], np.float32)
    keep = decode_ref.circle_nms(dets, 1.5, 83)
    assert list(keep) == [3, 0, 2]


def test_full_model_decode_runs():
    """End to end: forward + get_bboxes on the small config, compared with the oracle on the HIP maps."""
    from sgv3d_amd.models.bev_height import BEVHeight
    bc, hc = S.small_conf(depth=18)
    torch.manual_seed(0)
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 1)
    with torch.no_grad():                                    # make some heat rise above the 0.1 threshold
        for th in m.head.task_heads:
            th.heatmap[1].bias.fill_(-1.0)
            th.heatmap[1].weight.mul_(3.0)
    m = m.to(DEV)
    imgs, mats = S.make_images(2, bc['final_dim'], device=DEV, seed=4), S.make_mats(2, device=DEV, scale=128 / 864)
    with torch.no_grad():
        preds = m(imgs, mats)
        res = m.get_bboxes(preds, [dict(), dict()])
    preds_cpu = tuple([{k: v.cpu().numpy() for k, v in p[0].items()}] for p in preds)
    ref = decode_ref.get_bboxes(preds_cpu, hc['bbox_coder'], hc['test_cfg'], m.head.num_classes)
    for i in range(2):
        assert res[i][0].tensor.shape == ref[i][0].shape
        np.testing.assert_allclose(res[i][0].tensor.cpu().numpy(), ref[i][0], rtol=1e-3, atol=1e-3)
        assert np.array_equal(res[i][2].cpu().numpy(), ref[i][2])


def test_single_task_entry_is_the_batched_one():
    """sgv3d_centerpoint_decode (one task per call, the round-1 ABI) and sgv3d_centerpoint_decode_tasks (all tasks in three
    launches, what get_bboxes calls) give the same bytes."""
    import ctypes
    from sgv3d_amd import _lib
    from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead
    _, hc = S.r50_256_conf()
    head = BEVHeightHead(**hc)
    B, H, W, K = 2, 128, 128, 500
    buf, layout = _fake_preds(B, H, W, seed=77)
    dbuf = torch.from_numpy(buf).to(DEV)
    lib = _lib.load()
    T = len(layout)
    coder, tcfg = hc['bbox_coder'], hc['test_cfg']
    rng_c = (ctypes.c_float * 6)(*[float(v) for v in coder['post_center_range']])
    outs = []
    for t, d in enumerate(layout):
        p = {k: dbuf[:, o:o + c] for k, (o, c) in d.items()}
        cat = p['heatmap'].shape[1]
        nws = lib.sgv3d_centerpoint_decode_workspace_bytes(B, cat, K)
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        o = dict(boxes=torch.empty(B, K, 9, device=DEV), scores=torch.empty(B, K, device=DEV),
                 labels=torch.empty(B, K, dtype=torch.int32, device=DEV), valid=torch.empty(B, K, dtype=torch.uint8, device=DEV),
                 keep=torch.empty(B, K, dtype=torch.uint8, device=DEV))
        rc = lib.sgv3d_centerpoint_decode(B, cat, H, W, K, p['heatmap'].data_ptr(), p['reg'].data_ptr(), p['height'].data_ptr(),
                                          p['dim'].data_ptr(), p['rot'].data_ptr(), p['vel'].data_ptr(), int(dbuf.stride(0)),
                                          float(coder['out_size_factor']), float(coder['voxel_size'][0]), float(coder['voxel_size'][1]),
                                          float(coder['pc_range'][0]), float(coder['pc_range'][1]), float(coder['score_threshold']),
                                          rng_c, 1, float(tcfg['min_radius'][t]), int(tcfg['post_max_size']), ws.data_ptr(), nws,
                                          o['boxes'].data_ptr(), o['scores'].data_ptr(), o['labels'].data_ptr(), o['valid'].data_ptr(),
                                          o['keep'].data_ptr(), _lib.stream_handle(torch.device(DEV)))
        _lib.check(rc, "sgv3d_centerpoint_decode")
        outs.append(o)
    preds = tuple([{k: dbuf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)
    res = head.get_bboxes(preds, img_metas=[dict() for _ in range(B)])
    torch.cuda.synchronize()
    for i in range(B):
        want_b, want_s, want_l, off = [], [], [], 0
        for t, o in enumerate(outs):
            k = o['keep'][i].bool()
            bb = o['boxes'][i][k].clone()
            bb[:, 2] = bb[:, 2] - bb[:, 5] * 0.5
            want_b.append(bb); want_s.append(o['scores'][i][k]); want_l.append(o['labels'][i][k] + off)
            off += head.num_classes[t]
        assert torch.equal(res[i][0].tensor, torch.cat(want_b)) and torch.equal(res[i][1], torch.cat(want_s))
        assert torch.equal(res[i][2], torch.cat(want_l).int())


# ---------------------------------------------------------------------------------------------------------------------
# Ties, mask and NMS edges, kernel forms, argument checks and rounding of the circle decode: inputs, known answers and the raw
# C-ABI call live in tests/decode_circle_ref.py; tests/test_decode_circle_cpu.py checks on the CPU that the inputs have the
# ties and edges they are meant to have.
@functools.lru_cache(maxsize=None)
def _shared_head():
    from sgv3d_amd.layers.heads.bev_height_head import BEVHeightHead
    _, hc = S.r50_256_conf()
    return BEVHeightHead(**hc)


def _head(ncls, coder, tcfg, norm_bbox=True):
    """A head whose decode is configured for one case (get_bboxes reads nothing else of the module)."""
    head = _shared_head()
    head.num_classes, head.bbox_coder_cfg, head.norm_bbox = list(ncls), coder, norm_bbox
    head.test_cfg = dict(tcfg, nms_type='circle')
    return head


def _merged(dbuf, layout, coder, tcfg, ncls, norm_bbox=True):
    head = _head(ncls, coder, tcfg, norm_bbox)
    res = head.get_bboxes(C.preds_of(dbuf, layout), img_metas=[dict() for _ in range(dbuf.shape[0])])
    return [[r[0].tensor.cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy()] for r in res]


_worst = dict(scores=0.0, dim=0.0, rot=0.0, z=0.0)       # the largest deviations seen in the toleranced columns


def _close(name, got, want, **tol):
    if got.size:
        with np.errstate(invalid='ignore'):
            _worst[name] = max(_worst[name], float(np.nanmax(np.abs(got.astype(np.float64) - want, dtype=np.float64), initial=0.0)))
    np.testing.assert_allclose(got, want, **tol)


def _check_raw(raw, ref, has_vel=True):
    """All K rows of every (task, sample): order, cells and decisions exact, the transcendental columns within tolerance."""
    assert np.array_equal(raw['labels'], ref['labels'])
    assert np.array_equal(raw['valid'], ref['valid'])
    assert np.array_equal(raw['keep'], ref['keep'])
    exact = [0, 1, 2, 7, 8]                                   # x, y, height, vel
    assert np.array_equal(raw['boxes'][..., exact], ref['boxes'][..., exact], equal_nan=True)
    _close('scores', raw['scores'], ref['scores'], rtol=1e-5, atol=1e-6)
    _close('dim', raw['boxes'][..., 3:6], ref['boxes'][..., 3:6], rtol=1e-3, atol=1e-3)
    _close('rot', raw['boxes'][..., 6], ref['boxes'][..., 6], rtol=1e-3, atol=1e-3)
    if not has_vel:
        assert not raw['boxes'][..., 7:].any()


def _check_merged(res, ref):
    assert len(res) == len(ref)
    for (boxes, scores, labels), (rb, rs, rl) in zip(res, ref):
        assert boxes.shape == rb.shape and boxes.shape[1] == 9, (boxes.shape, rb.shape)      # per-sample counts
        assert labels.dtype == np.int32 and np.array_equal(labels, rl)
        assert np.array_equal(boxes[:, [0, 1, 7, 8]], rb[:, [0, 1, 7, 8]], equal_nan=True)   # row order, x, y, vel
        _close('scores', scores, rs, rtol=1e-5, atol=1e-6)
        _close('z', boxes[:, 2], rb[:, 2], rtol=1e-3, atol=1e-3)                             # height - dim2 / 2
        _close('dim', boxes[:, 3:6], rb[:, 3:6], rtol=1e-3, atol=1e-3)
        _close('rot', boxes[:, 6], rb[:, 6], rtol=1e-3, atol=1e-3)


def _report():
    print("largest deviations so far:", {k: "%.3g" % v for k, v in _worst.items()})


def _run_both(buf, layout, coder, tcfg, ncls, norm_bbox=True, dbuf=None):
    dbuf = torch.from_numpy(buf).to(DEV) if dbuf is None else dbuf
    rc, raw = C.raw_decode(dbuf, layout, coder, tcfg, norm_bbox)
    assert rc == 0
    res = _merged(dbuf, layout, coder, tcfg, ncls, norm_bbox)
    return raw, res


@pytest.mark.parametrize("case", C.TIE_CASES, ids=lambda c: "%dx%d-K%d" % c[:3])
def test_ties_match_oracle(case):
    """Quantised heat: the K-th score of every class sits inside a group of equal scores and classes share scores, so the
    'lower flat index, then lower class' rule decides which cells are reported and in which order."""
    buf, layout, coder, tcfg, ncls = C.tie_case(case)
    raw, res = _run_both(buf, layout, coder, tcfg, ncls)
    _check_raw(raw, C.oracle_raw(buf, layout, coder, tcfg))
    _check_merged(res, C.oracle_merged(buf, layout, coder, tcfg, ncls))
    _report()


def test_ties_unaligned_storage_and_rerun_are_bitwise():
    """The 64 x 64 tie case from storage that is only 4-byte aligned (scalar loads although H*W % 4 == 0), and twice from the
    aligned one: the same bytes each time."""
    case = C.TIE_CASES[2]
    assert case[:3] == (64, 64, 512)
    buf, layout, coder, tcfg, ncls = C.tie_case(case)
    dbuf = torch.from_numpy(buf).to(DEV)
    flat = torch.zeros(buf.size + 4, dtype=torch.float32, device=DEV)
    shifted = flat[1:1 + buf.size].view(buf.shape)
    shifted.copy_(dbuf)
    assert dbuf.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    runs = [_run_both(buf, layout, coder, tcfg, ncls, dbuf=d) for d in (dbuf, dbuf, shifted)]
    _check_raw(runs[0][0], C.oracle_raw(buf, layout, coder, tcfg))
    for raw, res in runs[1:]:
        for k in raw:
            assert raw[k].tobytes() == runs[0][0][k].tobytes(), k
        for a, b in zip(res, runs[0][1]):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("K", C.EDGE_KS)
def test_edges_known_answers(K):
    """score > thr (strict), centre range (inclusive, NaN out), dist <= radius^2 (inclusive), chain suppression, and the cap
    counting kept boxes only: the reported centres are the hand-worked answers, in order; all rows are the oracle's."""
    for name, (buf, layout, coder, tcfg, want) in C.edge_cases(K).items():
        raw, res = _run_both(buf, layout, coder, tcfg, [1])
        got = [tuple(float(v) for v in row[:2]) for row in res[0][0]]
        assert got == [tuple(float(v) for v in w) for w in want], (name, got, want)
        _check_raw(raw, C.oracle_raw(buf, layout, coder, tcfg))
        _check_merged(res, C.oracle_merged(buf, layout, coder, tcfg, [1]))


@pytest.mark.parametrize("H,W,K", C.DENSE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("cap", [83, 1 << 20])
def test_dense_nms_without_masks(H, W, K, cap):
    """No score threshold (-inf) and no centre range (null pointer): all K rows are valid, four radii, with and without a cap."""
    buf, layout, coder, tcfg, ncls = C.dense_case(H, W, K, cap)
    raw, res = _run_both(buf, layout, coder, tcfg, ncls)
    assert raw['valid'].all()
    ref = C.oracle_raw(buf, layout, coder, tcfg)
    print("survivors per task:", raw['keep'].sum((1, 2)).tolist(), "oracle:", ref['keep'].sum((1, 2)).tolist())
    _check_raw(raw, ref)
    _check_merged(res, C.oracle_merged(buf, layout, coder, tcfg, ncls))
    _report()


def test_dense_everything_kept_fills_the_packed_buffer():
    """reg = 0, one class per task, radius 0, no cap: distinct cells have distinct centres, so all T*K rows of a sample are
    reported -- the packed output is written to its last row."""
    H, W, K = C.DENSE_SHAPES[0]
    buf, layout, coder, tcfg, ncls = C.dense_case(H, W, K, 1 << 20, ncls=(1, 1, 1, 1), reg_zero=True, radii=[0.0] * 4)
    raw, res = _run_both(buf, layout, coder, tcfg, ncls)
    assert raw['keep'].all()
    assert all(r[0].shape == (4 * K, 9) for r in res)
    _check_raw(raw, C.oracle_raw(buf, layout, coder, tcfg))
    _check_merged(res, C.oracle_merged(buf, layout, coder, tcfg, ncls))


def test_dense_without_vel_and_norm_bbox():
    """No ``vel`` map (columns 7 and 8 are zero) and ``norm_bbox`` off (``dim`` is copied, not exponentiated)."""
    H, W, K = C.DENSE_SHAPES[1]
    buf, layout, coder, tcfg, ncls = C.dense_case(H, W, K, 83, has_vel=False)
    raw, res = _run_both(buf, layout, coder, tcfg, ncls, norm_bbox=False)
    ref = C.oracle_raw(buf, layout, coder, tcfg, norm_bbox=False)
    _check_raw(raw, ref, has_vel=False)
    assert np.array_equal(raw['boxes'][..., 3:6], ref['boxes'][..., 3:6])          # copied through
    merged = C.oracle_merged(buf, layout, coder, tcfg, ncls, norm_bbox=False)
    _check_merged(res, merged)
    assert all(not r[0][:, 7:].any() and len(r[0]) for r in res)


def test_sample_without_detections():
    buf, layout, coder, tcfg, want = C.empty_case()
    raw, res = _run_both(buf, layout, coder, tcfg, [1])
    assert not raw['valid'][0, 0].any() and not raw['keep'][0, 0].any()
    assert res[0][0].shape == (0, 9) and res[0][1].shape == (0,) and res[0][2].shape == (0,)
    assert [tuple(float(v) for v in row[:2]) for row in res[1][0]] == [tuple(w) for w in want[1]]
    _check_raw(raw, C.oracle_raw(buf, layout, coder, tcfg))
    _check_merged(res, C.oracle_merged(buf, layout, coder, tcfg, [1]))


def test_rejections_before_any_launch():
    """Arguments the kernels cannot handle are refused by the entry: a non-zero code, and not a byte of the outputs written."""
    buf, layout, coder, tcfg, _ = C.edge_cases(8)['chain']
    dbuf = torch.from_numpy(buf).to(DEV)
    many = dict(tcfg, min_radius=[1.0] * 17)
    calls = {
        'K = 1025': dict(coder=dict(coder, max_num=1025)),
        'K > H*W': dict(coder=dict(coder, max_num=C.EDGE_H * C.EDGE_W + 1)),
        '17 tasks': dict(layout=layout * 17, tcfg=many),
        'a task without a class': dict(layout=layout * 2, tcfg=many, ncls=[1, 0]),
        'workspace one byte short': dict(ws_delta=-1),
    }
    for name, kw in calls.items():
        rc, raw = C.raw_decode(dbuf, kw.get('layout', layout), kw.get('coder', coder), kw.get('tcfg', tcfg),
                               ncls=kw.get('ncls'), ws_delta=kw.get('ws_delta', 0))
        assert rc != 0, name
        for k, v in raw.items():
            assert (v.view(np.uint8) == C.POISON).all(), (name, k)
    rc, raw = C.raw_decode(dbuf, layout, coder, tcfg)                             # and the same call, valid, is accepted
    assert rc == 0 and raw['keep'].sum() == 2


def test_rounding_parity_nms_decisions():
    """Shipped coder (0.4 m cells from -51.2 m), task 0's radius^2 = 4: pairs of peaks in one column, 5 rows (2.0 m) apart,
    at the rows where one fused multiply-add in ``y = t * voxel + pc`` moves y by an ulp and the pair's ``dist <= 4`` with
    it (tests/decode_circle_ref.rounding_pairs).  ``keep`` must be the oracle's: one rounding per operation."""
    _, hc = S.r50_256_conf()
    radius = hc['test_cfg']['min_radius'][0]
    pairs, tried, _ = C.rounding_pairs(hc['bbox_coder'], radius)
    assert pairs
    rows = [p[0] for p in pairs[:12]]
    buf, layout, coder, cells = C.rounding_field(hc['bbox_coder'], rows)
    assert max(c for _, c in cells) - min(c for _, c in cells) >= 20
    tcfg = dict(min_radius=[radius], post_max_size=83)
    raw, res = _run_both(buf, layout, coder, tcfg, [1])
    ref = C.oracle_raw(buf, layout, coder, tcfg)
    differ = int((raw['keep'] != ref['keep']).sum())
    y_off = int((raw['boxes'][..., 1] != ref['boxes'][..., 1]).sum())
    print("%d pairs of %d candidates placed (rows %s): keep differs in %d rows, y differs bitwise in %d of %d rows" %
          (len(rows), len(pairs), rows, differ, y_off, raw['keep'].size))
    assert differ == 0
    _check_raw(raw, ref)
    _check_merged(res, C.oracle_merged(buf, layout, coder, tcfg, [1]))


def test_rounding_parity_centres_on_a_continuous_field():
    """Random continuous maps, shipped coder: x, y, z of all K rows of every task are bitwise the oracle's."""
    _, hc = S.r50_256_conf()
    H, W, B, K = 64, 96, 1, 500
    buf, layout = _fake_preds(B, H, W, seed=H)
    coder = dict(hc['bbox_coder'], max_num=K)
    rc, raw = C.raw_decode(torch.from_numpy(buf).to(DEV), layout, coder, hc['test_cfg'])
    assert rc == 0
    ref = C.oracle_raw(buf, layout, coder, hc['test_cfg'])
    off = (raw['boxes'][..., :3] != ref['boxes'][..., :3])
    print("rows whose x / y / z differ bitwise:", off.reshape(-1, 3).sum(0).tolist(), "of", off[..., 0].size)
    assert np.array_equal(raw['labels'], ref['labels'])
    assert not off.any()
    assert np.array_equal(raw['valid'], ref['valid']) and np.array_equal(raw['keep'], ref['keep'])
