"""The device AP evaluator on the MI355X: the kernels against their host twin bit for bit, ``kitti_eval_device`` against
``kitti_eval`` and the reference's golden text, guard bands, repeatability, the copy count, and the evaluator's switch."""
import os

import numpy as np
import pytest
import torch

import device_eval_util as U
import kitti_chain_util as K
from sgv3d_amd import _lib, hip_ops
from sgv3d_amd.evaluators import device_eval as DE
from sgv3d_amd.evaluators.kitti_utils.eval import _rboxes, kitti_eval
from sgv3d_amd.evaluators.kitti_utils.rotate_iou import rotate_iou_pairs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 4096
SETS = {}


def _set(name):
    """(gts, dts, classes, float32 BEV / 3-D overlaps of the existing kernel, host-twin curves), computed once per set."""
    if name not in SETS:
        if name == 'golden':
            gts, dts = U.golden_annos()
            classes = [0, 1, 2]
        elif name == 'stress':
            gts, dts = U.stress_set(3)
            classes = [0, 1, 2, 3]
        else:
            gts, dts = U.crossing_set()
            classes = [0, 2]
        flat = []
        for metric in (1, 2):
            ov = rotate_iou_pairs([_rboxes(d, metric) for d in dts], [_rboxes(g, metric) for g in gts], -1, DEV)
            flat.append(np.concatenate([o.reshape(-1) for o in ov]).astype(np.float32))
        mo = U.MIN_OVERLAPS[:, :, classes]
        packed = DE.pack_annotations(gts, dts, pinned=True)
        SETS[name] = dict(gts=gts, dts=dts, classes=classes, mo=mo, packed=packed,
                          twin=DE.curves_host(packed, flat[0], flat[1], classes, mo, True))
    return SETS[name]


def _launch(s, ws_slack=0, fill=0x5A):
    """The C entry on buffers with guard bands: -> (rc, outputs region bytes, whole device buffer on the host, layout)."""
    lib, pk, C = _lib.load(), s['packed'], len(s['classes'])
    offs, out_bytes = DE._out_layout(18 * C)
    ws = lib.sgv3d_kitti_eval_device_workspace_bytes(pk.M, pk.TG, pk.TD, pk.pairs, C)
    in_bytes = (pk.buffer.numel() + 7) // 8 * 8
    o_out, o_ws = GUARD + in_bytes + GUARD, GUARD + in_bytes + GUARD + out_bytes + GUARD
    total = o_ws + ws + GUARD
    dbuf = torch.full((total,), fill, dtype=torch.uint8, device=DEV)
    dbuf[GUARD:GUARD + pk.buffer.numel()].copy_(pk.buffer)
    classes = np.ascontiguousarray(s['classes'], np.int32)
    mo = np.ascontiguousarray(s['mo'], np.float64)
    base = dbuf.data_ptr()
    with torch.cuda.device(DEV):
        rc = lib.sgv3d_kitti_eval_device(pk.M, pk.TG, pk.TD, pk.pairs, pk.tiles, base + GUARD, pk.buffer.numel(), C, classes.ctypes.data,
                                         mo.ctypes.data, 1, base + o_ws, ws + ws_slack, *[base + o_out + o for o in offs],
                                         _lib.stream_handle(torch.device(DEV)))
        torch.cuda.synchronize()
    host = dbuf.cpu().numpy()
    return rc, host[o_out:o_out + out_bytes], host, (in_bytes, o_out, out_bytes, o_ws, ws)


@pytest.mark.parametrize("name", ["golden", "stress", "crossing"])
def test_kernels_match_the_host_twin_and_leave_the_guard_bands(name):
    s = _set(name)
    rc, raw, host, (in_bytes, o_out, out_bytes, o_ws, ws) = _launch(s)
    assert rc == 0
    got = DE._split_outputs(raw, len(s['classes']))
    assert got[4] == 0 and s['twin'][4] == 0
    U.assert_curves(got, s['twin'])
    if name == 'crossing':
        assert s['packed'].TG == 1040 and s['twin'][3][:, 0].max() == 41          # 1040 true positives in the Car cells
    for lo, hi in ((0, GUARD), (GUARD + in_bytes, o_out), (o_out + out_bytes, o_ws), (o_ws + ws, len(host))):
        assert (host[lo:hi] == 0x5A).all(), (lo, hi)
    assert host[GUARD:GUARD + s['packed'].buffer.numel()].tobytes() == s['packed'].buffer.numpy().tobytes()     # the input is read only
    # a repeat launch gives the same bytes, whatever the workspace held before
    rc2, raw2, _, _ = _launch(s, fill=0xC3)
    used = DE._out_layout(18 * len(s['classes']))[0][4] + 4                          # (the region ends with four bytes of padding)
    assert rc2 == 0 and raw2[:used].tobytes() == raw[:used].tobytes()


def test_short_workspace_is_refused_before_any_launch():
    s = _set('stress')
    rc, raw, host, (in_bytes, o_out, out_bytes, o_ws, ws) = _launch(s, ws_slack=-8)
    assert rc == -3 and b"needed" in _lib.load().sgv3d_last_error()
    assert (host[o_out:] == 0x5A).all()                                            # nothing ran


def test_an_image_with_too_many_detections_sets_the_status_bit_and_counts_as_empty(monkeypatch):
    """A caller that packs by other means than ``pack_annotations``: nothing faults, status bit 1 says so, and the curves are
    those of the set with that image's detections removed."""
    gts, dts = U.stress_set(2, images=3)
    gts[1] = U._anno(np.random.default_rng(5), 7, U.GT_NAMES, False)
    crowd = U._anno(np.random.default_rng(6), DE.MAX_DETECTIONS + 1, U.DT_NAMES, True)
    classes = [0, 1, 2]
    mo = U.MIN_OVERLAPS[:, :, classes]
    monkeypatch.setattr(DE, 'MAX_DETECTIONS', 1 << 20)
    packed = DE.pack_annotations(gts, [dts[0], crowd, dts[2]], pinned=True)
    monkeypatch.undo()
    rc, raw, host, _ = _launch(dict(packed=packed, classes=classes, mo=mo))
    assert rc == 0
    got = DE._split_outputs(raw, len(classes))
    assert got[4] == 2
    empty = U._anno(np.random.default_rng(6), 0, U.DT_NAMES, True)
    thinned = [dts[0], empty, dts[2]]
    flat = []
    for metric in (1, 2):
        ov = rotate_iou_pairs([_rboxes(d, metric) for d in thinned], [_rboxes(g, metric) for g in gts], -1, DEV)
        flat.append(np.concatenate([o.reshape(-1) for o in ov]).astype(np.float32))
    U.assert_curves(got, DE.curves_host(DE.pack_annotations(gts, thinned), flat[0], flat[1], classes, mo, True))
    with pytest.raises(RuntimeError, match="4096"):
        DE._check_status(got[4])


def _synthetic(frames=12, seed=9):
    """Cars, pedestrians and cyclists with jittered detections, misses, false positives and DontCare regions."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(frames):
        n = int(rng.integers(3, 12))
        x1, y1 = rng.uniform(0, 1500, n), rng.uniform(100, 700, n)
        w, h = rng.uniform(40, 200, n), rng.uniform(20, 150, n)
        g = {'name': rng.choice(['Car', 'Car', 'Pedestrian', 'Cyclist', 'Van', 'DontCare'], n).astype('<U14'),
             'truncated': rng.choice([0.0, 0.2, 0.4], n), 'occluded': rng.choice([0.0, 1.0, 2.0], n), 'alpha': rng.uniform(-3, 3, n),
             'bbox': np.stack([x1, y1, x1 + w, y1 + h], 1), 'dimensions': np.stack([rng.uniform(1, 4.5, n), rng.uniform(1.4, 1.9, n), rng.uniform(0.6, 1.9, n)], 1),
             'location': np.stack([rng.uniform(-30, 30, n), rng.uniform(0.8, 1.4, n), rng.uniform(10, 90, n)], 1),
             'rotation_y': rng.uniform(-3, 3, n), 'score': np.zeros(n)}
        keep = rng.uniform(size=n) < 0.85
        d = {k: v[keep].copy() for k, v in g.items()}
        m = int(keep.sum())
        d['name'] = np.array(['Car' if x in ('Van', 'DontCare') else x for x in d['name']], dtype='<U14')
        d['bbox'] += rng.normal(0, 3, (m, 4))
        d['location'] += rng.normal(0, 0.15, (m, 3))
        d['rotation_y'] += rng.normal(0, 0.05, m)
        d['alpha'] += rng.normal(0, 0.1, m)
        d['score'] = np.round(rng.uniform(0.1, 1, m), 2)
        d['truncated'], d['occluded'] = np.zeros(m), np.zeros(m)
        gts.append(g)
        dts.append(d)
    return gts, dts


def _assert_same_report(got, want):
    assert list(got[1]) == list(want[1])
    for k in want[1]:
        assert np.asarray(got[1][k]).tobytes() == np.asarray(want[1][k]).tobytes(), k
    assert got[0] == want[0]


@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_kitti_eval_device_equals_kitti_eval(name):
    gts, dts = U.golden_annos() if name == 'golden' else _synthetic()
    classes = ['Car', 'Pedestrian', 'Cyclist']
    want = kitti_eval(gts, dts, classes)
    got = DE.kitti_eval_device(gts, dts, classes, device=DEV)
    assert "aos" in want[0] and max(v for k, v in want[1].items() if '_3D_' in k) > 10.0       # a set with real matches
    _assert_same_report(got, want)
    if name == 'golden':                                      # the reference's own text and values
        assert got[0] == str(U.GOLD['result_text'])
        vals = dict(zip([str(k) for k in U.GOLD['ret_keys']], U.GOLD['ret_vals']))
        assert set(vals) == set(got[1])
        for k, v in vals.items():
            assert abs(got[1][k] - v) < 1e-9, k
    # one metric, the 11-point AP, a pre-packed ground truth and a single class go the same way
    _assert_same_report(DE.kitti_eval_device(DE.pack_ground_truth(gts), dts, 'Car', eval_types=('3d',), metric='R11', device=DEV),
                        kitti_eval(gts, dts, 'Car', eval_types=('3d',), metric='R11'))


def test_one_upload_one_download_no_wait_in_between():
    from torch.profiler import ProfilerActivity, profile
    gts, dts = U.golden_annos()
    DE.kitti_eval_device(gts, dts, ['Car', 'Pedestrian', 'Cyclist'], device=DEV)        # warm: ground truth packed, allocator
    saved, hip_ops.PROFILE = hip_ops.PROFILE, []
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            DE.kitti_eval_device(gts, dts, ['Car', 'Pedestrian', 'Cyclist'], device=DEV)
            torch.cuda.synchronize()
        labels = [r[0] for r in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = saved
    copies = [e.name for e in prof.events() if 'memcpy' in e.name.lower()]
    print("copies:", sorted(set(copies)))
    squash = lambda c: c.lower().replace(' ', '')
    assert labels == ["kitti_eval_device", "kitti_curves_to_host"], labels
    assert len([c for c in copies if 'dtoh' in squash(c)]) == 1, copies
    assert len([c for c in copies if 'htod' in squash(c)]) == 1, copies
    # the only wait of the call is the one after the download (the profiled region's own device-wide wait comes on top)
    waits = [e.name for e in prof.events() if e.name in ('hipStreamSynchronize', 'hipEventSynchronize')]
    print("waits:", waits)
    assert len(waits) <= 1, waits


def test_evaluate_detections_device_eval_switch(tmp_path, capsys):
    from sgv3d_amd.evaluators import RoadSideEvaluator
    from sgv3d_amd.evaluators.device_kitti import KittiDetections
    root = K.kitti_root(tmp_path)
    toks = K.tokens()
    metas = K.metas_for(toks)
    boxes, scores, labels, counts = K.random_detections(3, 40, [40, 33, 17], seed=4)
    results = K.as_results(boxes, scores, labels, counts)
    # ground truth derived from the detections: some dropped, the rest moved a little
    rng = np.random.default_rng(6)
    gt = []
    for b, s, l in results:
        keep = rng.uniform(size=len(s)) < 0.8
        gb = b[keep].copy()
        gb[:, :2] += rng.normal(0, 0.1, (len(gb), 2)).astype(np.float32)
        gt.append((gb, np.ones(len(gb), np.float32), l[keep]))
    raw = K.file_chain(gt, metas, root, tmp_path / 'gt_raw')
    os.makedirs(tmp_path / 'gt')
    for sid in K.GOLD['calib_ids']:
        lines = open(os.path.join(raw, f'{int(sid):06d}.txt')).read().splitlines()
        (tmp_path / 'gt' / f'{int(sid):06d}.txt').write_text("".join(" ".join(ln.split(' ')[:15]) + "\n" for ln in lines))
    ev = RoadSideEvaluator(class_names=K.CLASS_NAMES, current_classes=["Car", "Pedestrian", "Cyclist"], data_root=root,
                           gt_label_path=str(tmp_path / 'gt'))
    out = {}
    for flag in (False, True):
        dets = KittiDetections(K.CLASS_NAMES, data_root=root)
        dets.add(results, metas)
        capsys.readouterr()
        value = ev.evaluate_detections(dets, metric_path=str(tmp_path / f'metrics_{flag}'), device_eval=flag)
        out[flag] = (value, capsys.readouterr().out, sorted(os.listdir(tmp_path / f'metrics_{flag}' / 'R40')))
    assert out[True] == out[False]
    assert out[True][0] > 1.0 and "Car AP@" in out[True][1]
    name = out[True][2][0]
    assert open(tmp_path / 'metrics_True' / 'R40' / name).read() == open(tmp_path / 'metrics_False' / 'R40' / name).read()
