"""GPU: detections -> KITTI annotations on the device (csrc/result2kitti.hip, evaluators/device_kitti.py) against the
reference's own label files, against the host entry that shares the kernel's per-detection function, against the
kernel's contract (rows beyond the counts, guard bands, repeatability, overflow, workspace), on real ``decode_device``
buffers and in a closed evaluation loop against ``RoadSideEvaluator.evaluate``."""
import json
import os

import numpy as np
import pytest
import torch

import kitti_chain_util as U
from sgv3d_amd import _lib, hip_ops, synthetic as S
from sgv3d_amd.evaluators.device_kitti import KittiDetections
from sgv3d_amd.evaluators.kitti_utils import kitti_common as KC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                           # bytes of 0xA5 before and after every output region


def assert_annos_equal(got, want):
    """Key by key, dtype by dtype, bit by bit."""
    (ga, gi), (wa, wi) = got, want
    assert gi == wi and len(ga) == len(wa)
    for g, w in zip(ga, wa):
        assert set(g) == set(w)
        for k in w:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (k, g[k].dtype, w[k].dtype, g[k].shape, w[k].shape)
            assert g[k].tobytes() == w[k].tobytes(), k


def device_entry(det, calib, max_det, digits, table=U.TABLE, expect=0, short_workspace=False):
    """sgv3d_detections_to_kitti over device copies of numpy arrays -> (kept, cls, fields) with the regions pre-filled
    with 0xA5 bytes; the guard bands around them are checked here."""
    lib = _lib.load()
    boxes, scores, labels, counts = det
    B, N = scores.shape
    f64 = boxes.dtype == np.float64
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (boxes, scores, labels, counts, calib)]
    sizes = [B * max_det * 13 * 8, B * max_det * 4, B * 4]
    offs, total = [], GUARD
    for s in sizes:
        offs.append(total)
        total += (s + 7) // 8 * 8 + GUARD
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    nws = lib.sgv3d_detections_to_kitti_workspace_bytes(B, N)
    assert nws == B * N * 4
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    p = out.data_ptr()
    rc = lib.sgv3d_detections_to_kitti(B, N, d[0].data_ptr(), d[1].data_ptr(), int(f64), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                       table.ctypes.data, len(table), U.THR, U.IMG[0], U.IMG[1], max_det, digits, ws.data_ptr(),
                                       nws - 4 if short_workspace else nws, p + offs[0], p + offs[1], p + offs[2],
                                       _lib.stream_handle(torch.device(DEV)))
    assert rc == expect, (rc, lib.sgv3d_last_error())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    used = np.zeros(total, bool)
    for o, s in zip(offs, sizes):
        used[o:o + s] = True
    assert np.all(raw[~used] == 0xA5), "a guard band was written"
    fields = raw[offs[0]:offs[0] + sizes[0]].view(np.float64).reshape(B, max_det, 13)
    cls = raw[offs[1]:offs[1] + sizes[1]].view(np.int32).reshape(B, max_det)
    kept = raw[offs[2]:offs[2] + sizes[2]].view(np.int32)
    return kept, cls, fields, raw


@pytest.fixture(scope="module")
def kitti_calibs(tmp_path_factory):
    root = U.kitti_root(tmp_path_factory.mktemp("calib"))
    return root, U.fixture_calibs(root)


# --------------------------------------------------------------------------------------------------------- golden text
def test_fixture_through_add_and_write_gives_the_reference_files(tmp_path):
    """The reference's own label files, through the public interface; the JSON's doubles go in as float64 tensors."""
    root = U.kitti_root(tmp_path)
    empty_id = 999                                                        # a frame without detections
    first = f"{int(U.GOLD['calib_ids'][0]):06d}.txt"
    calib_dir = os.path.join(root, 'training', 'calib')
    open(os.path.join(calib_dir, f'{empty_id:06d}.txt'), 'w').write(open(os.path.join(calib_dir, first)).read())
    res = json.loads(str(U.GOLD['results_json']))['results']
    toks = U.tokens()
    results = []
    for t in toks:
        rows = [list(p['translation']) + [p['size'][1], p['size'][0], p['size'][2], p['box_yaw'], 0.0, 0.0] for p in res[t]]
        results.append([torch.tensor(rows, dtype=torch.float64, device=DEV),
                        torch.tensor([p['detection_score'] for p in res[t]], dtype=torch.float64, device=DEV),
                        torch.tensor([U.CLASS_NAMES.index(p['detection_name']) for p in res[t]], device=DEV)])
    results.append([torch.zeros(0, 9, dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV),
                    torch.zeros(0, dtype=torch.int64, device=DEV)])
    metas = U.metas_for(toks + [f'training/image_2/{empty_id:06d}.jpg'])
    dets = KittiDetections(U.CLASS_NAMES, data_root=root)
    dets.add(results[:2], metas[:2])                                      # two calls: batches of two
    dets.add(results[2:], metas[2:])
    folder = dets.write(str(tmp_path / 'out'))
    assert folder == str(tmp_path / 'out' / 'data')
    for sid, want in zip(U.GOLD['calib_ids'], U.GOLD['label_text']):
        assert open(os.path.join(folder, f'{int(sid):06d}.txt')).read() == str(want), int(sid)
    assert open(os.path.join(folder, f'{empty_id:06d}.txt')).read() == ""
    want = KC.get_label_annos(folder, return_ids=True)
    assert want[1] == sorted([int(s) for s in U.GOLD['calib_ids']] + [empty_id])
    assert_annos_equal(dets.annos(), want)
    assert want[0][-1]['name'].shape == (0,) and want[0][-1]['bbox'].shape == (0, 4)


def test_cpu_tensors_are_refused():
    dets = KittiDetections(U.CLASS_NAMES)
    with pytest.raises(RuntimeError, match="GPU"):
        dets.add_packed(torch.zeros(44 * 4 + 4, dtype=torch.uint8), U.metas_for(U.tokens()[:1]), calib=[(np.eye(4), np.eye(3))])


# ------------------------------------------------------------------------------------------------- device against host
def _shape_case(name):
    if name == "b3_n96":
        return U.random_detections(3, 96, (0, 17, 96), seed=11), 96
    if name == "b1_n3000":                               # 498 rows: two chunks of one workgroup width; more than 256 kept
        det = U.random_detections(1, 3000, (498,), seed=12)
        det[1][:] = np.minimum(det[1] + np.float32(0.3), np.float32(0.99))
        return det, 498
    return U.random_detections(8, 96, (96, 1, 64, 65, 0, 33, 95, 7), seed=13), 96


@pytest.mark.parametrize("case", ["b3_n96", "b1_n3000", "b8_n96"])
def test_kernel_matches_the_host_entry(case, kitti_calibs):
    det, max_det = _shape_case(case)
    B = len(det[3])
    calibs = [kitti_calibs[1][b % 3] for b in range(B)]
    calib = U.calib_blocks(calibs, U.metas_for(['t'] * B))
    hk, hc, hf = U.host_entry(*det, calib, max_det, -1)
    dk, dc, df, _ = device_entry(det, calib, max_det, -1)
    assert np.array_equal(dk, hk) and dk.max() <= max_det
    if case == "b1_n3000":
        assert dk[0] > 256
    worst = 0.0
    for b in range(B):
        m = hk[b]
        assert np.array_equal(dc[b, :m], hc[b, :m])
        assert np.array_equal(df[b, :m, 12], hf[b, :m, 12])                          # the scores: row order
        if m:
            worst = max(worst, float(np.abs(df[b, :m] - hf[b, :m]).max()))
    print(f"{case}: kept {dk.tolist()}, unrounded max |device - host| = {worst:.3e}")
    assert worst <= 1e-9
    _, hc4, hf4 = U.host_entry(*det, calib, max_det, 4)
    dk4, dc4, df4, _ = device_entry(det, calib, max_det, 4)
    assert np.array_equal(dk4, hk)
    sel = [(b, slice(0, hk[b])) for b in range(B) if hk[b]]
    share = U.assert_rounded_alike(np.concatenate([df4[b, s] for b, s in sel]), np.concatenate([hf4[b, s] for b, s in sel]),
                                   np.concatenate([hf[b, s] for b, s in sel]))
    print(f"{case}: {share * 100:.3f} % of the values within {U.BOUNDARY} of a rounding boundary")


# ------------------------------------------------------------------------------------------------------------ contract
def test_kernel_contract(kitti_calibs):
    det, _ = _shape_case("b3_n96")
    boxes, scores, labels, counts = det
    calib = U.calib_blocks(kitti_calibs[1], U.metas_for(U.tokens()))
    kept, cls, fields, raw = device_entry(det, calib, 96, 4)
    assert kept[0] == 0 and kept[2] > 20
    # rows at and beyond counts[b]: NaN boxes and scores, huge labels -- never read
    pb, ps, pl = boxes.copy(), scores.copy(), labels.copy()
    for b in range(3):
        pb[b, counts[b]:], ps[b, counts[b]:], pl[b, counts[b]:] = np.nan, np.nan, 2 ** 31 - 1
    pl[1, counts[1]:counts[1] + 3] = -2 ** 31
    _, _, _, raw_poisoned = device_entry((pb, ps, pl, counts), calib, 96, 4)
    assert raw_poisoned.tobytes() == raw.tobytes()
    # a second launch: the same bytes (no atomics on the output)
    assert device_entry(det, calib, 96, 4)[3].tobytes() == raw.tobytes()
    # a cap below kept: the true count, intact rows below the cap, nothing beyond it (the guard bands are checked inside)
    cap = 5
    k5, c5, f5, _ = device_entry(det, calib, cap, 4)
    assert np.array_equal(k5, kept) and k5[2] > cap
    for b in range(3):
        m = min(int(kept[b]), cap)
        assert np.array_equal(c5[b, :m], cls[b, :m]) and f5[b, :m].tobytes() == fields[b, :m].tobytes()
        assert np.all(c5[b, m:].view(np.uint8) == 0xA5)
    # a short workspace is refused (SGV3D_ENOSPACE), nothing is written
    ks, _, _, _ = device_entry(det, calib, 96, 4, expect=-3, short_workspace=True)
    assert np.all(ks.view(np.uint8) == 0xA5)
    # the same overflow through the class: annos() raises, naming the frame and the count
    dets = KittiDetections(U.CLASS_NAMES, max_det=cap)
    dets.add([[torch.from_numpy(a).to(DEV) for a in r] for r in U.as_results(*det)], U.metas_for(U.tokens()), calib=kitti_calibs[1])
    first = next(b for b in range(3) if kept[b] > cap)
    with pytest.raises(RuntimeError, match=rf"{int(U.GOLD['calib_ids'][first]):06d}\.jpg.*: {int(kept[first])} detections .*max_det is {cap}"):
        dets.annos()


# ------------------------------------------------------------------------------------- real decode buffers, closed loop
N_FRAMES = 12


def _calib_text(c):
    P2 = np.zeros((3, 4))
    P2[:3, :3] = c['intrin'][:3, :3]
    tr = np.linalg.inv(c['sensor2ego'].astype(np.float64))[:3]
    return "P2: " + " ".join(f"{v:.6f}" for v in P2.reshape(-1)) + "\n" + \
           "Tr_velo_to_cam: " + " ".join(f"{v:.8f}" for v in tr.reshape(-1)) + "\n"


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The synthetic scene set of test_closed_loop_ap_gpu.py (HIP chain only): the small model with heads that fire, twelve
    frames with their own cameras, a KITTI-layout root with their calibration files, and the head's maps."""
    from sgv3d_amd.models.bev_height import BEVHeight
    tmp = tmp_path_factory.mktemp("scene")
    bc, hc = S.small_conf(final=(128, 192), bev=64, depth=18)
    hc['bbox_coder'] = dict(hc['bbox_coder'], pc_range=[0, -12.8, -5, 25.6, 12.8, 3], post_center_range=[0.0, -15.0, -10.0, 30.0, 15.0, 10.0],
                            max_num=100)
    hc['test_cfg'] = dict(hc['test_cfg'], post_center_limit_range=[0.0, -15.0, -10.0, 30.0, 15.0, 10.0], post_max_size=20)
    old = hip_ops.AUTOTUNE
    hip_ops.AUTOTUNE = False
    try:
        torch.manual_seed(0)
        m = BEVHeight(bc, hc).eval()
        S.checkpoint_like_(m, 2)
        with torch.no_grad():
            for t in m.head.task_heads:
                t.heatmap[1].weight.mul_(40.0)
                t.heatmap[1].bias.fill_(-1.0)
                t.dim[1].weight.mul_(3.0)
                t.dim[1].bias.fill_(0.6)
                t.height[1].bias.fill_(-0.5)
        imgs = torch.cat([S.make_images(1, bc['final_dim'], seed=100 + i) for i in range(N_FRAMES)])
        cams = [S.make_calib(pitch_deg=11.0 + (i % 3), cam_h=5.5 + 0.3 * (i % 2), fx=2183.375 * 192 / 1536, fy=2329.2976 * 128 / 864,
                             cx=940.59 * 192 / 1536, cy=567.568 * 128 / 864) for i in range(N_FRAMES)]
        t = lambda k: torch.from_numpy(np.stack([c[k] for c in cams])).view(N_FRAMES, 1, 1, 4, 4)
        mats = {'sensor2ego_mats': t('sensor2ego'), 'intrin_mats': t('intrin'), 'ida_mats': t('ida'),
                'sensor2sensor_mats': torch.eye(4).view(1, 1, 1, 4, 4).repeat(N_FRAMES, 1, 1, 1, 1),
                'sensor2virtual_mats': t('sensor2virtual'),
                'reference_heights': torch.tensor([float(c['reference_height']) for c in cams]).view(N_FRAMES, 1, 1),
                'bda_mat': torch.eye(4).repeat(N_FRAMES, 1, 1)}
        m = m.to(DEV)
        m.graph_forward = False
        with torch.no_grad():
            preds = m(imgs.to(DEV), {k: v.to(DEV) for k, v in mats.items()})
        torch.cuda.synchronize()
    finally:
        hip_ops.AUTOTUNE = old
    root = tmp / 'dair-v2x-i-kitti'
    os.makedirs(root / 'training' / 'calib')
    metas = []
    for i, c in enumerate(cams):
        full = dict(c, intrin=np.diag([1536 / 192, 864 / 128, 1, 1]).astype(np.float32) @ c['intrin'] / 0.8)
        full['intrin'][2, 2] = 1.0
        (root / 'training' / 'calib' / f'{i:06d}.txt').write_text(_calib_text(full))
        metas.append(dict(token=f'training/image_2/{i:06d}.jpg', ego2global_translation=[0, 0, 0], ego2global_rotation=[1, 0, 0, 0]))
    return dict(model=m, preds=preds, metas=metas, root=str(root), tmp=tmp)


def _labels_and_copies(fn):
    """The project's profiler labels of the launches ``fn`` makes, and the device -> host copies torch's profiler sees."""
    from torch.profiler import ProfilerActivity, profile
    saved = hip_ops.PROFILE
    hip_ops.PROFILE = []
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        labels = [r[0] for r in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = saved
    copies = [e.name for e in prof.events() if 'memcpy' in e.name.lower()]
    print("copies:", sorted(set(copies)))
    return labels, [c for c in copies if 'dtoh' in c.lower().replace(' ', '')]


@pytest.mark.parametrize("nms_type", ["circle", "rotate"])
def test_add_packed_on_a_decode_buffer_equals_add_of_get_bboxes(scene, nms_type):
    m, metas = scene['model'], scene['metas']
    old = m.head.test_cfg
    m.head.test_cfg = dict(old, nms_type=nms_type)
    try:
        with torch.no_grad():
            packed = m.head.decode_device(scene['preds'])
            results = m.head.get_bboxes(scene['preds'], metas, decoded=packed)
    finally:
        m.head.test_cfg = old
    n_det = sum(len(r[1]) for r in results)
    assert n_det > 5 * N_FRAMES, n_det
    a, b = KittiDetections(S.CLASSES, data_root=scene['root']), KittiDetections(S.CLASSES, data_root=scene['root'])
    a.add_packed(packed, metas)                                  # (warm: calibration files read, pinned buffer allocated)
    labels, d2h = _labels_and_copies(lambda: a.add_packed(packed, metas))
    # one launch and one copy to the host, of the annotations: the raw boxes never cross
    assert labels == ["detections_to_kitti", "kitti_annos_to_host"], labels
    assert len(d2h) == 1, d2h
    b.add(results, metas)
    b.add(results, metas)
    got, want = a.annos(), b.annos()
    assert_annos_equal(got, want)
    kept = sum(len(x['name']) for x in got[0])
    print(f"{nms_type}: {n_det} detections, {kept // 2} kept")
    assert 0 < kept // 2 < n_det and got[1] == list(range(N_FRAMES))
    # frames that share a token are concatenated in arrival order: both calls' rows, twice the same
    for x in got[0]:
        n = len(x['name']) // 2
        assert x['bbox'][:n].tobytes() == x['bbox'][n:].tobytes() and np.array_equal(x['index'], np.arange(2 * n))


def test_closed_loop_evaluate_detections_equals_evaluate(scene):
    from sgv3d_amd.evaluators import RoadSideEvaluator
    m, metas, tmp, root = scene['model'], scene['metas'], scene['tmp'], scene['root']
    with torch.no_grad():
        packed = m.head.decode_device(scene['preds'])
        results = m.head.get_bboxes(scene['preds'], metas, decoded=packed)
    host = [(r[0].tensor.cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy()) for r in results]
    # ground truth derived from the detections: a fifth dropped, the rest jittered, so that the AP table is not degenerate
    rng = np.random.default_rng(5)
    gt_dets = []
    for b, s, l in host:
        keep = (s > 0.45) & (rng.uniform(size=len(s)) < 0.8)
        gb = b[keep].copy()
        gb[:, :2] += rng.normal(0, 0.15, (len(gb), 2)).astype(np.float32)
        gb[:, 6] += rng.normal(0, 0.05, len(gb)).astype(np.float32)
        gt_dets.append((gb, np.ones(len(gb), np.float32), l[keep]))
    classes = ["Car", "Pedestrian", "Cyclist"]
    ev = RoadSideEvaluator(class_names=S.CLASSES, current_classes=classes, data_root=root, gt_label_path=str(tmp / 'gt'))
    gt_raw = U.file_chain(gt_dets, metas, root, tmp / 'gt_raw', class_names=S.CLASSES)
    os.makedirs(tmp / 'gt')
    for i in range(N_FRAMES):                                               # ground-truth files: no score column
        lines = open(os.path.join(gt_raw, f'{i:06d}.txt')).read().splitlines()
        (tmp / 'gt' / f'{i:06d}.txt').write_text("".join(" ".join(ln.split(' ')[:15]) + "\n" for ln in lines))
    want = ev.evaluate(host, metas, jsonfile_prefix=str(tmp / 'json'), results_path=str(tmp / 'out'), metric_path=str(tmp / 'metrics_files'))
    dets = KittiDetections(S.CLASSES, data_root=root)
    dets.add_packed(packed, metas)
    got = ev.evaluate_detections(dets, metric_path=str(tmp / 'metrics_device'))
    assert got == want and 1.0 < got < 99.0, (got, want)
    name = 'epoch_result_{}.txt'.format(round(want, 2))
    text_files = open(tmp / 'metrics_files' / 'R40' / name).read()
    assert open(tmp / 'metrics_device' / 'R40' / name).read() == text_files and "Car" in text_files
    assert_annos_equal(dets.annos(), KC.get_label_annos(str(tmp / 'out' / 'data'), return_ids=True))
    # and the files it writes are the file chain's files
    folder = dets.write(str(tmp / 'out_device'))
    for i in range(N_FRAMES):
        assert open(os.path.join(folder, f'{i:06d}.txt')).read() == open(tmp / 'out' / 'data' / f'{i:06d}.txt').read(), i
