"""GPU: the renderer's three kernels (csrc/render.hip) against the host twin that shares their geometry and coverage functions,
byte for byte: hand-placed boxes (tests/render_ref.py: in view, across each frame edge, across the near plane, behind the
camera, far outside the guard rectangle, zero extents, NaN, the score threshold, an unmapped class, overlapping classes, labels
over predictions) at thickness 1, 2, 3, with and without canvas and masks, in and out of place, on 40 x 64, 37 x 61 and
130 x 260 frames at batch 1 and 3; the kernel contract (guard bands, untouched tiles, a 0xFF workspace, repeatability, overflow,
a short workspace); ``draw_packed`` on a real ``decode_device`` buffer; graph capture; the annotate path into the JPEG encoder."""
import ctypes
import io

import numpy as np
import pytest
import torch

import render_ref as R
from sgv3d_amd import _lib, hip_ops, render, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                                          # bytes of 0xA5 before and after every output region


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class DeviceCall:
    """sgv3d_render_detections over device copies of a scene, outputs inside 0xA5 guard bands, the workspace pre-filled 0xFF."""

    def __init__(self, sc, cfg, masks, in_place, labels=True, shift=0):
        self.lib = _lib.load()
        B, H, W = sc['frames'].shape[:3]
        self.shape, self.cfg = (B, H, W), cfg
        f64 = sc['boxes'].dtype == np.float64
        self.m = sc['label_rows'].shape[1] if labels else 0
        self.desc = R.make_desc(cfg, B, sc['boxes'].shape[1], self.m, H, W, f64)
        self.t = {k: _dev(sc[k]) for k in ('boxes', 'scores', 'labels', 'counts', 'calib')}
        self.t['label_rows'] = _dev(sc['label_rows']) if labels else None
        self.t['label_counts'] = _dev(sc['label_counts']) if labels else None
        self.t['masks'] = _dev(sc['masks']) if masks else None
        fbytes = B * H * W * 3
        bbytes = B * cfg['bev']['h'] * cfg['bev']['w'] * 3 if cfg['bev'] else 0
        up = lambda n: (n + 15) // 16 * 16
        # shift: the frames and the canvas start that many bytes off a 16-byte boundary (the byte path of odd bases)
        self.off_out, self.off_bev, self.off_status = GUARD + shift, 2 * GUARD + up(fbytes) + 16 + shift, 3 * GUARD + up(fbytes) + up(bbytes) + 48
        self.sizes = (fbytes, bbytes, B * 4)
        self.buf = torch.full((self.off_status + up(B * 4) + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.in_place = in_place
        if in_place:
            self.buf[self.off_out:self.off_out + fbytes] = _dev(sc['frames']).reshape(-1)
            self.t['frames'] = None
        else:
            self.t['frames'] = _dev(sc['frames'])
            if shift:                                            # the source on an odd base too
                self.src = torch.empty(fbytes + 16, dtype=torch.uint8, device=DEV)
                self.src[shift:shift + fbytes] = self.t['frames'].reshape(-1)
                self.t['frames'] = self.src[shift:shift + fbytes]
        self.nws = self.lib.sgv3d_render_workspace_bytes(ctypes.byref(self.desc))
        assert self.nws > 0
        self.work = torch.full((self.nws,), 0xFF, dtype=torch.uint8, device=DEV)

    def launch(self, workspace_bytes=None, expect=0):
        p = self.buf.data_ptr()
        P = _lib.ptr
        frames = p + self.off_out if self.in_place else self.t['frames'].data_ptr()
        rc = self.lib.sgv3d_render_detections(
            ctypes.byref(self.desc), P(self.t['boxes']), P(self.t['scores']), P(self.t['labels']), P(self.t['counts']), P(self.t['calib']),
            P(self.t['label_rows']), P(self.t['label_counts']), frames, P(self.t['masks']), p + self.off_out,
            p + self.off_bev if self.cfg['bev'] else None, p + self.off_status, self.work.data_ptr(),
            self.nws if workspace_bytes is None else workspace_bytes, _lib.stream_handle(torch.device(DEV)))
        assert rc == expect, (rc, self.lib.sgv3d_last_error())
        return self

    def read(self):
        """-> (out, bev, status) and the raw buffer; the guard bands are checked here."""
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        used = np.zeros(raw.size, bool)
        for o, s in zip((self.off_out, self.off_bev, self.off_status), self.sizes):
            used[o:o + s] = True
        assert np.all(raw[~used] == 0xA5), "a guard band was written"
        B, H, W = self.shape
        out = raw[self.off_out:self.off_out + self.sizes[0]].reshape(B, H, W, 3)
        bev = raw[self.off_bev:self.off_bev + self.sizes[1]].reshape(B, self.cfg['bev']['h'], self.cfg['bev']['w'], 3) if self.cfg['bev'] else None
        return out, bev, raw[self.off_status:self.off_status + self.sizes[2]].view(np.int32)


def _twin(sc, cfg, masks, in_place, labels=True):
    lab = (sc['label_rows'], sc['label_counts']) if labels else (None, None)
    return R.host_twin(cfg, sc['boxes'], sc['scores'], sc['labels'], sc['counts'], sc['calib'], sc['frames'], *lab,
                       sc['masks'] if masks else None, in_place)


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("frames", "bev", "status")):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape, (what, name)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {name} differs at {len(bad)} bytes, first {bad[:4].tolist()}")


@pytest.mark.parametrize("batch", R.BATCHES)
@pytest.mark.parametrize("hw", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_match_the_host_twin_byte_for_byte(hw, batch):
    drawn = 0
    for dtype in (np.float32, np.float64):
        sc = R.scene(hw[0], hw[1], batch, dtype)
        for t, bev, masks, in_place in R.variants():
            if dtype is np.float64 and (t != 2 or in_place):
                continue
            cfg = R.config(t, bev)
            got = DeviceCall(sc, cfg, masks, in_place).launch().read()
            want = _twin(sc, cfg, masks, in_place)
            _assert_same(got, want, (dtype.__name__, t, bev, masks, in_place))
            assert not got[2].any()
            drawn += int((got[0] != sc['frames']).any(-1).sum())
    assert drawn > 500 * batch


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_frames_and_canvas_on_odd_bases(shift):
    """Output (and source) pointers that are not 4-byte aligned: the paint kernel's byte path on a width that is a multiple of 4."""
    sc = R.scene(40, 64, 3)
    cfg = R.config(2, True)
    for masks, in_place in ((True, False), (False, True)):
        call = DeviceCall(sc, cfg, masks, in_place, shift=shift)
        assert (call.buf.data_ptr() + call.off_out) % 4 == shift and (call.buf.data_ptr() + call.off_bev) % 4 == shift
        _assert_same(call.launch().read(), _twin(sc, cfg, masks, in_place), f"shift {shift}, masks {masks}, in place {in_place}")


def test_without_labels_and_with_an_empty_sample():
    sc = R.scene_empty_sample()
    cfg = R.config(2, True)
    got = DeviceCall(sc, cfg, False, False, labels=False).launch().read()
    _assert_same(got, _twin(sc, cfg, False, False, labels=False), "no labels")
    assert np.array_equal(got[0][1], sc['frames'][1]) and not got[1][1].any() and got[1][0].any()


def test_in_place_leaves_untouched_tiles_alone_and_a_relaunch_is_bitwise():
    """In place, a pixel no primitive covers keeps its bytes: with frames of one value, every byte is that value or a colour
    the twin put there; the 0xFF workspace and the guard bands are checked by DeviceCall.  A second launch on the drawn frame
    (the lines are idempotent) and a repeat out of place give the same bytes."""
    sc = R.scene_constant()
    cfg = R.config(2, True)
    call = DeviceCall(sc, cfg, False, True).launch()
    first = [a.copy() for a in call.read()]
    want = _twin(sc, cfg, False, True)
    _assert_same(first, want, "in place")
    untouched = ~(want[0] != 0x5B).any(-1)
    assert untouched.mean() > 0.5 and np.all(first[0][untouched] == 0x5B)
    _assert_same(call.launch().read(), first, "relaunch in place")
    out_of_place = DeviceCall(sc, cfg, False, False)
    a = [x.copy() for x in out_of_place.launch().read()]
    b = out_of_place.launch().read()
    _assert_same(a, first, "out of place against in place")
    _assert_same(b, a, "relaunch out of place")


def test_overflow_copies_that_frame_through_and_draws_the_others():
    sc = R.scene(40, 64, 3)
    cfg = R.config(2, True, max_boxes=9)
    sc['counts'][1] = 9
    for in_place in (False, True):
        got = DeviceCall(sc, cfg, True, in_place).launch().read()
        _assert_same(got, _twin(sc, cfg, True, in_place), f"overflow, in place {in_place}")
        assert got[2].tolist() == [R.EOVERFLOW, 0, R.EOVERFLOW]
        assert np.array_equal(got[0][0], sc['frames'][0]) and np.array_equal(got[0][2], sc['frames'][2])
        assert not got[1][0].any() and got[1][1].any() and (got[0][1] != sc['frames'][1]).any()
    sc['label_counts'][:] = [0, 3, 0]
    sc['counts'][:] = 1
    cfg = R.config(2, False, max_boxes=2)
    got = DeviceCall(sc, cfg, False, False).launch().read()
    _assert_same(got, _twin(sc, cfg, False, False), "label overflow")
    assert got[2].tolist() == [0, R.EOVERFLOW, 0]


def test_a_workspace_one_byte_short_is_refused():
    sc = R.scene(40, 64, 1)
    call = DeviceCall(sc, R.config(2, True), False, False)
    call.launch(workspace_bytes=call.nws - 1, expect=-3)
    assert b"workspace" in call.lib.sgv3d_last_error()
    out, bev, status = call.read()
    assert np.all(out == 0xA5) and np.all(bev == 0xA5)               # nothing was launched


def test_capture_in_a_graph_and_replay_on_new_boxes():
    sc = R.scene(37, 61, 3)
    cfg = R.config(2, True)
    call = DeviceCall(sc, cfg, True, False)
    call.launch()                                                    # warm: code objects loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call.launch()
    other = R.scene_replay()
    for k in ('boxes', 'scores', 'labels', 'counts', 'frames', 'masks'):
        call.t[k].copy_(_dev(other[k]))
    call.buf[call.off_out:call.off_out + call.sizes[0]] = 0xA5
    g.replay()
    got = call.read()
    want = _twin(other, cfg, True, False)
    _assert_same(got, want, "graph replay")
    assert not np.array_equal(want[0], _twin(sc, cfg, True, False)[0])


# ------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture(scope="module")
def decoded():
    """The small model with heads that fire on two synthetic frames, its 'circle' decode buffer and the cameras."""
    from sgv3d_amd.models.bev_height import BEVHeight
    n = 2
    bc, hc = S.small_conf(final=(128, 192), bev=64, depth=18)
    hc['bbox_coder'] = dict(hc['bbox_coder'], pc_range=[0, -12.8, -5, 25.6, 12.8, 3], post_center_range=[0.0, -15.0, -10.0, 30.0, 15.0, 10.0],
                            max_num=100)
    hc['test_cfg'] = dict(hc['test_cfg'], post_center_limit_range=[0.0, -15.0, -10.0, 30.0, 15.0, 10.0], post_max_size=20, nms_type='circle')
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
        imgs = torch.cat([S.make_images(1, bc['final_dim'], seed=100 + i) for i in range(n)])
        cams = [S.make_calib(pitch_deg=11.0 + i, cam_h=5.5 + 0.3 * i, fx=2183.375 * 192 / 1536, fy=2329.2976 * 128 / 864,
                             cx=940.59 * 192 / 1536, cy=567.568 * 128 / 864) for i in range(n)]
        t = lambda k: torch.from_numpy(np.stack([c[k] for c in cams])).view(n, 1, 1, 4, 4)
        mats = {'sensor2ego_mats': t('sensor2ego'), 'intrin_mats': t('intrin'), 'ida_mats': t('ida'),
                'sensor2sensor_mats': torch.eye(4).view(1, 1, 1, 4, 4).repeat(n, 1, 1, 1, 1), 'sensor2virtual_mats': t('sensor2virtual'),
                'reference_heights': torch.tensor([float(c['reference_height']) for c in cams]).view(n, 1, 1),
                'bda_mat': torch.eye(4).repeat(n, 1, 1)}
        m = m.to(DEV)
        m.graph_forward = False
        with torch.no_grad():
            preds = m(imgs.to(DEV), {k: v.to(DEV) for k, v in mats.items()})
            packed = m.head.decode_device(preds)
            results = m.head.get_bboxes(preds, [{} for _ in range(n)], decoded=packed)
        torch.cuda.synchronize()
    finally:
        hip_ops.AUTOTUNE = old
    calib = [(np.linalg.inv(c['sensor2ego'].astype(np.float64))[:3], c['intrin'][:3, :3].astype(np.float64)) for c in cams]
    metas = [dict(token=f'{i:06d}', ego2global_translation=[0, 0, 0], ego2global_rotation=[1, 0, 0, 0]) for i in range(n)]
    return dict(packed=packed, results=results, calib=calib, metas=metas, n=n)


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
    names = [e.name for e in prof.events()]
    kernels = [n for n in names if 'render_' in n and 'kernel' in n]
    return labels, kernels, [n for n in names if 'memcpy' in n.lower() and 'dtoh' in n.lower().replace(' ', '')]


def test_draw_packed_on_a_decode_buffer(decoded):
    H, W = 128, 192
    n, packed, metas, calib = decoded['n'], decoded['packed'], decoded['metas'], decoded['calib']
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(DEV)
    canvas = render.BevCanvas(side_range=(-15, 15), fwd_range=(0, 30), res=0.25)
    r = render.DetectionRenderer(S.CLASSES, src_hw=(H, W), max_boxes=128, bev=canvas, score_threshold=0.1)
    r.draw_packed(frames, packed, metas, calib=calib)                # warm
    box = {}
    labels, kernels, d2h = _labels_and_copies(lambda: box.setdefault('out', r.draw_packed(frames, packed, metas, calib=calib)))
    assert labels == ["render_detections"], labels
    assert len(kernels) == 3 and [sum(name in k for k in kernels) for name in ('render_setup_kernel', 'render_bin_kernel', 'render_paint_kernel')] == [1, 1, 1], kernels
    assert d2h == [], d2h                                            # nothing crosses to the host before status()
    out = box['out']
    assert out.status().tolist() == [0] * n
    # the same through draw() on get_bboxes' lists and through the host twin on the buffer's own bytes
    via_lists = r.draw(frames, decoded['results'], metas, calib=calib)
    assert torch.equal(via_lists.frames, out.frames) and torch.equal(via_lists.bev, out.bev)
    raw = packed.cpu().numpy()
    N = (raw.size - 4 * n) // (44 * n)
    boxes = raw[:n * N * 36].view(np.float32).reshape(n, N, 9)
    scores = raw[n * N * 36:n * N * 40].view(np.float32).reshape(n, N)
    cls = raw[n * N * 40:n * N * 44].view(np.int32).reshape(n, N)
    counts = raw[n * N * 44:].view(np.int32)
    cfg = dict(R.config(2, False, max_boxes=128), score_thr=0.1, table=render.class_table(S.CLASSES, render.category_map_dair),
               class_colors=render.default_class_colors(S.CLASSES).tolist(),
               bev=dict(w=canvas.width, h=canvas.height, res=canvas.res, x_off=canvas.x_off, y_off=canvas.y_off))
    want = R.host_twin(cfg, boxes, scores, cls, counts, np.stack([render.calib_block(*c) for c in calib]), frames.cpu().numpy())
    assert np.array_equal(out.frames.cpu().numpy(), want[0]) and np.array_equal(out.bev.cpu().numpy(), want[1])
    kept = int(sum(((scores[b, :counts[b]] > 0.1) & (cfg['table'][cls[b, :counts[b]]] >= 0)).sum() for b in range(n)))
    print(f"draw_packed: {int(counts.sum())} detections, {kept} kept, {int((want[0] != frames.cpu().numpy()).any(-1).sum())} pixels drawn")
    assert kept >= 4 and (want[0] != frames.cpu().numpy()).any() and want[1].any()
    # in place
    mine = frames.clone()
    same = r.draw_packed(mine, packed, metas, calib=calib, out=mine)
    assert same.frames.data_ptr() == mine.data_ptr() and torch.equal(mine, out.frames)


def test_annotated_frames_through_the_jpeg_encoder_and_back(decoded):
    """draw_packed -> JpegEncoder -> JpegDecoder against Pillow's decode of the same bytes."""
    from PIL import Image
    from sgv3d_amd.jpeg import JpegDecoder
    from sgv3d_amd.jpeg_encode import JpegEncoder
    H, W = 128, 192
    n = decoded['n']
    y, x = np.mgrid[0:H, 0:W]
    scene = np.stack([100 + 50 * np.sin(x / 23.0), 90 + 0.7 * y, 160 - 0.4 * x], -1) + np.random.default_rng(4).normal(0, 4, (n, H, W, 3))
    frames = torch.from_numpy(np.clip(scene, 0, 255).astype(np.uint8)).to(DEV)
    r = render.DetectionRenderer(S.CLASSES, src_hw=(H, W), max_boxes=128, score_threshold=0.1)
    out = r.draw_packed(frames, decoded['packed'], decoded['metas'], calib=decoded['calib'])
    files = JpegEncoder(src_hw=(H, W), quality=95, subsampling='4:4:4', max_bytes=1 << 18)(out.frames).files()
    back = JpegDecoder(src_hw=(H, W), max_bytes=1 << 18, device=DEV)(files)
    torch.cuda.synchronize()
    pil = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert('RGB')) for f in files])
    assert np.array_equal(back.cpu().numpy(), pil)
    drawn = (out.frames != frames).any(-1).cpu().numpy()
    assert drawn.sum() > 50
