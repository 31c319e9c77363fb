"""CPU: the host side of the renderer (csrc/render.hip, sgv3d_amd/render.py): the C ABI and every rejection by name, the host
twin against the numpy restatement of the contract (tests/render_ref.py) bit for bit on every case the GPU tests run, the
reference's own corners, ``pcl2xy_plane`` integers and label boxes (tests/golden/render.npz), the two properties that tie the
line rule to Pillow's lines, and known answers of the rule.  The kernels run the same functions (test_render_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import render_ref as R
from conftest import GOLDEN, ROOT
from sgv3d_amd import _lib, render

NEW = ("sgv3d_render_workspace_bytes", "sgv3d_render_detections", "sgv3d_render_detections_host")
GOLD = np.load(os.path.join(GOLDEN, "render.npz"))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def _header():
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NEW)
def test_header_and_ctypes_agree(name):
    m = re.search(r"([a-z_0-9]+)\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in sgv3d_hip.h"
    res, args = _lib._PROTOS[name]
    assert res == {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)]
    decl = [a.strip() for a in m.group(2).split(",")]
    assert len(decl) == len(args)
    for d, a in zip(decl, args):
        if "sgv3d_render_desc" in d:
            assert a == ctypes.POINTER(_lib.RenderDesc)
        elif "*" in d:
            assert a == ctypes.c_void_p
        else:
            assert a == {"size_t": ctypes.c_size_t, "int": ctypes.c_int}[d.split()[0]]
    assert hasattr(_lib.load(), name)


def test_descriptor_mirrors_the_header_struct():
    body = re.search(r"typedef struct \{([^}]*)\} sgv3d_render_desc;", _header()).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            n = n.strip()
            m = re.match(r"(\w+)\[(\d+)\]", n)
            fields.append((m.group(1), ctype, int(m.group(2))) if m else (n, ctype, 0))
    base = {"int": ctypes.c_int, "double": ctypes.c_double, "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8}
    want = [(n, base[t] * k if k else base[t]) for n, t, k in fields]
    got = list(_lib.RenderDesc._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, g), (_, w) in zip(got, want):
        assert ctypes.sizeof(g) == ctypes.sizeof(w) and (g is w or g._type_ is w._type_), n
    assert render.EOVERFLOW == R.EOVERFLOW == int(re.search(r"#define SGV3D_RENDER_EOVERFLOW (\d+)", _header()).group(1))
    assert render.MAX_SIDE == int(re.search(r"#define SGV3D_RENDER_MAX_SIDE (\d+)", _header()).group(1))
    assert render.MAX_BOXES == int(re.search(r"#define SGV3D_RENDER_MAX_BOXES (\d+)", _header()).group(1))


def _good(device, bev=True, m=2):
    """A complete valid call over small host arrays: (arrays kept alive, descriptor, ordered arguments after the descriptor)."""
    B, N, H, W = 2, 4, 12, 20
    cfg = R.config(2, bev, max_boxes=4)
    d = R.make_desc(cfg, B, N, m, H, W, False)
    a = dict(boxes=np.zeros((B, N, 9), np.float32), scores=np.zeros((B, N), np.float32), labels=np.zeros((B, N), np.int32),
             counts=np.zeros(B, np.int32), calib=np.zeros((B, 33)), label_boxes=np.zeros((B, max(m, 1), 7)),
             label_counts=np.zeros(B, np.int32), frames=np.zeros((B, H, W, 3), np.uint8), masks=np.zeros((B, H, W), np.uint8),
             out=np.zeros((B, H, W, 3), np.uint8), bev=np.zeros((B, 81, 49, 3), np.uint8), status=np.zeros(B, np.int32),
             work=np.zeros(1 << 16, np.int32))
    P = lambda k: a[k].ctypes.data
    args = dict(boxes=P('boxes'), scores=P('scores'), labels=P('labels'), counts=P('counts'), calib=P('calib'),
                label_boxes=P('label_boxes') if m else None, label_counts=P('label_counts') if m else None, frames=P('frames'),
                masks=P('masks'), out=P('out'), bev=P('bev') if bev else None, status=P('status'))
    if device:
        args.update(work=P('work'), work_bytes=a['work'].nbytes, stream=None)
    return a, d, args


def _call(fn, d, args):
    return fn(ctypes.byref(d) if d is not None else None, *args.values())


@pytest.mark.parametrize("device", [False, True], ids=["host_entry", "device_entry"])
def test_every_bad_argument_is_refused_before_any_launch(device):
    """Each call has exactly one bad argument, so none reaches a launch (there is no GPU here)."""
    lib = _lib.load()
    fn = lib.sgv3d_render_detections if device else lib.sgv3d_render_detections_host
    keep, d, good = _good(device)

    def refused(word, desc=None, **change):
        dd = _lib.RenderDesc.from_buffer_copy(d)
        for k, v in (desc or {}).items():
            setattr(dd, k, v)
        rc = _call(fn, dd, dict(good, **change))
        msg = lib.sgv3d_last_error() or b""
        assert rc == -1 and word.encode() in msg, (desc, list(change), rc, msg)                     # SGV3D_EINVAL

    for key in ('boxes', 'scores', 'labels', 'counts', 'calib', 'frames', 'out', 'status'):
        refused("null pointer", **{key: None})
    refused("label_boxes", label_boxes=None)
    refused("label_boxes", label_counts=None)
    refused("label_boxes", desc=dict(m=0))
    refused("bev pointer", bev=None)
    refused("bev pointer", desc=dict(bev_h=0, bev_w=0))
    for field, value, word in [('batch', 0, "bad size"), ('batch', -1, "bad size"), ('batch', 65536, "bad size"), ('n', 0, "bad size"),
                               ('m', -1, "bad size"), ('height', 0, "frame"), ('width', 8193, "frame"), ('height', 8193, "frame"),
                               ('bev_h', 0, "canvas"), ('bev_w', -3, "canvas"), ('bev_w', 8193, "canvas"), ('max_boxes', 0, "max_boxes"),
                               ('max_boxes', 1025, "max_boxes"), ('thickness', 0, "thickness"), ('thickness', 16, "thickness"),
                               ('f64_inputs', 2, "f64_inputs"), ('num_classes', 0, "num_classes"), ('num_classes', 65, "num_classes"),
                               ('mask_alpha', -1, "mask_alpha"), ('mask_alpha', 257, "mask_alpha"), ('score_thr', float('nan'), "score_thr"),
                               ('z_near', 0.0, "z_near"), ('z_near', float('inf'), "z_near"), ('bev_res', 0.0, "bev_res"),
                               ('bev_res', float('nan'), "bev_res")]:
        refused(word, desc={field: value})
    dd = _lib.RenderDesc.from_buffer_copy(d)
    dd.class_table[1] = 3
    assert _call(fn, dd, good) == -1 and b"class_table" in lib.sgv3d_last_error()
    assert _call(fn, None, good) == -1 and b"null descriptor" in lib.sgv3d_last_error()
    refused("misaligned", boxes=good['boxes'] + 2)
    refused("misaligned", calib=good['calib'] + 4)
    refused("misaligned", status=good['status'] + 1)
    refused("misaligned", label_boxes=good['label_boxes'] + 4)
    refused("f64_inputs", desc=dict(f64_inputs=-1))
    refused("partly overlaps", out=good['frames'] + 3)                                             # out shifted inside frames
    refused("overlaps masks", out=good['masks'])
    refused("bev overlaps", bev=good['frames'])
    refused("bev overlaps", bev=good['out'] + 8)
    if device:
        need = lib.sgv3d_render_workspace_bytes(ctypes.byref(d))
        assert 0 < need <= keep['work'].nbytes
        refused("null pointer", work=None)
        refused("misaligned", work=good['work'] + 2)
        rc = _call(fn, d, dict(good, work_bytes=need - 1))
        assert rc == -3 and b"workspace" in lib.sgv3d_last_error()                                 # SGV3D_ENOSPACE: one byte short
        bad = _lib.RenderDesc.from_buffer_copy(d)
        bad.width = 0
        assert lib.sgv3d_render_workspace_bytes(ctypes.byref(bad)) == 0 and lib.sgv3d_render_workspace_bytes(None) == 0
    else:
        assert _call(fn, d, good) == 0                                                             # the list itself is valid
        assert _call(fn, d, dict(good, out=good['frames'])) == 0                                   # in place is not an overlap
        assert _call(fn, d, dict(good, masks=None)) == 0
        _, d0, good0 = _good(False, bev=False, m=0)
        assert _call(fn, d0, good0) == 0


def test_workspace_bytes_is_the_documented_layout():
    lib = _lib.load()
    _, d, _ = _good(True)
    tiles = lambda h, w: ((h + 31) // 32) * ((w + 31) // 32)
    words = lambda e: (2 * d.max_boxes * e + 31) // 32
    per = d.n + 2 * d.max_boxes * 14 * 5 + 2 * d.max_boxes * 4 * 5 + 4 + words(14) * tiles(d.height, d.width) + words(4) * tiles(d.bev_h, d.bev_w)
    assert lib.sgv3d_render_workspace_bytes(ctypes.byref(d)) == per * 4 * d.batch


def test_python_layer_refuses_before_any_launch():
    names = R.CLASS_NAMES
    with pytest.raises(render.RenderError, match="src_hw"):
        render.DetectionRenderer(names, src_hw=(1080, 8193))
    with pytest.raises(render.RenderError, match="max_boxes"):
        render.DetectionRenderer(names, max_boxes=0)
    with pytest.raises(render.RenderError, match="thickness"):
        render.DetectionRenderer(names, thickness=16)
    with pytest.raises(render.RenderError, match="z_near"):
        render.DetectionRenderer(names, z_near=0)
    with pytest.raises(render.RenderError, match="mask_alpha"):
        render.DetectionRenderer(names, mask_alpha=300)
    with pytest.raises(render.RenderError, match="class_colors"):
        render.DetectionRenderer(names, class_colors=[(1, 2, 3)])
    with pytest.raises(render.RenderError, match="palette"):
        render.DetectionRenderer(names, palette=[(1, 2, 3)] * 6)
    with pytest.raises(render.RenderError, match="BevCanvas"):
        render.DetectionRenderer(names, bev=(1001, 1201))
    with pytest.raises(render.RenderError, match="sides"):
        render.BevCanvas(side_range=(-600, 600), res=0.1)
    r = render.DetectionRenderer(names, src_hw=(12, 20))
    frames, packed, metas = torch.zeros(1, 12, 20, 3, dtype=torch.uint8), torch.zeros(4 * 44 + 4, dtype=torch.uint8), [{'token': 'a'}]
    with pytest.raises(render.RenderError, match="on the GPU"):
        r.draw_packed(frames, packed, metas, calib=np.zeros((1, 33)))
    with pytest.raises(render.RenderError, match="on the GPU"):
        r.draw(frames, [[torch.zeros(0, 9), torch.zeros(0), torch.zeros(0, dtype=torch.long)]], metas, calib=np.zeros((1, 33)))
    with pytest.raises(render.RenderError, match="decode_device"):
        r.draw_packed(frames, torch.zeros(7, dtype=torch.uint8), metas)
    assert np.array_equal(render.default_class_colors(['car', 'bus', 'van', 'truck', 'pedestrian', 'cyclist', 'barrier']),
                          [(0, 255, 0), (255, 255, 0), (255, 255, 0), (255, 255, 0), (0, 255, 255), (255, 0, 0), (255, 255, 255)])
    c = render.BevCanvas()
    assert (c.height, c.width, c.x_off, c.y_off) == (1001, 1201, -600, 1000)


# ----------------------------------------------------------------------------------------------- twin against restatement
def _run_both(sc, cfg, masks, in_place, labels=True):
    lab = (sc['label_rows'], sc['label_counts']) if labels else (None, None)
    mk = sc['masks'] if masks else None
    got = R.host_twin(cfg, sc['boxes'], sc['scores'], sc['labels'], sc['counts'], sc['calib'], sc['frames'], *lab, mk, in_place)
    want = R.render(cfg, sc['boxes'], sc['scores'], sc['labels'], sc['counts'], sc['calib'], sc['frames'], *lab, mk)
    return got, want


@pytest.mark.parametrize("batch", R.BATCHES)
@pytest.mark.parametrize("hw", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_is_the_restatement_bit_for_bit(hw, batch):
    """Every (thickness, canvas, mask, in place) variant of the GPU tests' scenes; float32 and float64 inputs."""
    drawn = 0
    for dtype in (np.float32, np.float64):
        sc = R.scene(hw[0], hw[1], batch, dtype)
        for t, bev, masks, in_place in R.variants():
            if dtype is np.float64 and (t != 2 or in_place):
                continue
            (out, bv, status), (want_out, want_bv, want_status) = _run_both(sc, R.config(t, bev), masks, in_place)
            assert np.array_equal(status, want_status) and not status.any()
            assert np.array_equal(out, want_out), (dtype, t, bev, masks, in_place)
            if bev:
                assert np.array_equal(bv, want_bv) and bv.any()
            if not masks:
                drawn += int((out != sc['frames']).any(-1).sum())
    assert drawn > 500 * batch


def test_host_twin_is_the_restatement_on_the_single_test_scenes():
    """The scenes that only one GPU test each builds: an empty sample without labels, constant frames, the graph replay's."""
    for name, sc, cfg, masks, in_place, labels in R.extra_cases():
        (out, bv, status), (want_out, want_bv, want_status) = _run_both(sc, cfg, masks, in_place, labels=labels)
        assert np.array_equal(status, want_status), name
        assert np.array_equal(out, want_out) and np.array_equal(bv, want_bv), name
        assert (out != sc['frames']).any(), name


def test_scene_draws_what_its_rows_say():
    """The scene's hand-placed rows do what their comments claim (on the restatement's own intermediate values)."""
    H, W = 130, 260
    sc = R.scene(H, W, 1, np.float64)
    cal = sc['calib'][0]
    prims = [R.camera_prims(R.pred_corners(sc['boxes'][0, r], cal), cal, W, H, 0.5, 2, (1, 2, 3)) for r in range(len(R.SCENE_ROWS))]
    inside = lambda p: all(0 <= v[0] < W and 0 <= v[1] < H and 0 <= v[2] < W and 0 <= v[3] < H for v in p)
    assert len(prims[0]) == 14 and inside(prims[0])
    assert any(min(v[0], v[2]) < 0 for v in prims[1]) and any(max(v[0], v[2]) >= W for v in prims[2])
    assert any(min(v[1], v[3]) < 0 for v in prims[3]) and any(max(v[1], v[3]) >= H for v in prims[4])
    assert 0 < len(prims[5]) < 14                                    # the near plane drops edges wholly behind it and cuts others
    assert prims[6] == [] and prims[7] == [] and prims[9] == [] and prims[15] == []
    assert len(prims[8]) == 14 and len({v[:4] for v in prims[8]}) == 1 and prims[8][0][0:2] == prims[8][0][2:4]     # one point
    (out, _, _), _ = _run_both(sc, R.config(2, False), False, False, labels=False)
    # order: where the later box (bus, yellow) and the earlier one (car, green) both cover a pixel the later one owns it
    cfg = R.config(2, False)
    only = lambda rows: R.render(cfg, sc['boxes'][:, rows], sc['scores'][:, rows], sc['labels'][:, rows], np.array([len(rows)], np.int32),
                                 sc['calib'], np.zeros_like(sc['frames']))[0][0].any(-1)
    both = only([12]) & only([13])
    assert both.sum() > 10 and np.all(out[0][both] == (255, 255, 0))
    # the threshold row and the unmapped class draw nothing: leaving them out changes no pixel
    rows = [r for r in range(len(R.SCENE_ROWS)) if r not in (10, 11)]
    less = R.render(cfg, sc['boxes'][:, rows], sc['scores'][:, rows], sc['labels'][:, rows], np.array([len(rows)], np.int32), sc['calib'],
                    sc['frames'])[0]
    assert np.array_equal(less, out)


def test_overflow_copies_the_frame_through_and_draws_the_others():
    sc = R.scene(40, 64, 3)
    cfg = R.config(2, True, max_boxes=9)                             # the scene keeps 14 detections per sample
    sc['counts'][1] = 9                                              # ... and all of its first nine rows
    (out, bv, status), (want_out, want_bv, want_status) = _run_both(sc, cfg, True, False)
    assert status.tolist() == [R.EOVERFLOW, 0, R.EOVERFLOW] == want_status.tolist()
    assert np.array_equal(out, want_out) and np.array_equal(bv, want_bv)
    assert np.array_equal(out[0], sc['frames'][0]) and np.array_equal(out[2], sc['frames'][2]) and not bv[0].any() and not bv[2].any()
    assert (out[1] != sc['frames'][1]).any() and bv[1].any()
    sc['label_counts'][:] = [0, 3, 0]                                # labels are counted separately
    cfg = R.config(2, False, max_boxes=2)
    sc['counts'][:] = 1
    (out, _, status), (want_out, _, want_status) = _run_both(sc, cfg, False, False)
    assert status.tolist() == [0, R.EOVERFLOW, 0] == want_status.tolist() and np.array_equal(out, want_out)


# ------------------------------------------------------------------------------------------------------------ the reference
def test_corners_are_the_references_bit_for_bit():
    """``get_lidar_3d_8points([w, l, h], yaw, [x, y, z + h / 2])`` is ``box_corner`` of the bottom centre."""
    rows, want = GOLD['corner_inputs'], GOLD['corner_outputs']
    for r, w in zip(rows, want):
        ex, ey, h, yaw, x, y, zc = (np.float64(v) for v in r)
        zb = zc - h / np.float64(2)
        got = np.array([R.box_corner(k, ex, ey, h, R._cos(yaw), R._sin(yaw), x, y, zb) for k in range(8)])
        assert got.tobytes() == w.tobytes()


@pytest.mark.parametrize("tag", ["default", "small"])
def test_bev_integers_are_pcl2xy_planes(tag):
    side0, side1, fwd0, fwd1, res = GOLD[f'bev_{tag}_cfg']
    as_int = lambda v: int(v) if v == int(v) else float(v)
    cfg = R.bev_config((as_int(side0), as_int(side1)), (as_int(fwd0), as_int(fwd1)), float(res))
    canvas = render.BevCanvas((as_int(side0), as_int(side1)), (as_int(fwd0), as_int(fwd1)), float(res))
    assert (cfg['h'], cfg['w']) == tuple(GOLD[f'bev_{tag}_shape']) == (canvas.height, canvas.width)
    assert (cfg['x_off'], cfg['y_off']) == (canvas.x_off, canvas.y_off)
    for corners, wx, wy in zip(GOLD['corner_outputs'], GOLD[f'bev_{tag}_x'], GOLD[f'bev_{tag}_y']):
        pts = R.bev_points(corners, cfg['res'], cfg['x_off'], cfg['y_off'])
        assert [p[0] for p in pts] == wx[:4].tolist() and [p[1] for p in pts] == wy[:4].tolist()


def test_label_boxes_are_read_label_bboxes():
    """``box_corner`` of ``label_boxes``' rows against the corners ``read_label_bboxes`` returned for the same file.

    The bound is reasoned, not measured.  The reference forms the corners with an ``np.matrix`` product, which runs through the
    BLAS numpy was built with; its kernels may fuse ``s * lx + c * ly`` (one rounding instead of two), which ``box_corner``,
    shared verbatim with the KITTI conversion and rounding once per operation, must not.  Fusing removes the rounding of one
    product, at most 2^-53 of that product (at most 2^-53 * half the box diagonal); the two sums then round to neighbours at
    worst, and so do the sums with the centre: two more ulps at the magnitude of the result, which the centre's magnitude plus
    half the diagonal bounds.  Together: 2^-51 * (|centre coordinate| + half diagonal).  z has no product and is exact.  (On the
    fixture 2 of 96 coordinates differ, by one ulp each, in the row that takes the alpha > pi branch.)"""
    rows = render.label_boxes(str(GOLD['label_text']), GOLD['label_cam2lidar'])
    want = GOLD['label_corners']
    assert rows.shape == (4, 7) and want.shape == (4, 8, 3)          # five lines, one with zero dimensions
    differ = 0
    for r, w in zip(rows, want):
        got = np.array(R.label_corners(r))
        assert got[:, 2].tobytes() == w[:, 2].tobytes()
        half_diagonal = 0.5 * float(np.hypot(r[3], r[4]))
        for axis in (0, 1):
            bound = 2.0 ** -51 * (abs(float(r[axis])) + half_diagonal)
            assert np.abs(got[:, axis] - w[:, axis]).max() <= bound
        differ += int((got != w).sum())
    print(f"label corners: {differ} of {want.size} coordinates differ from the reference's")
    assert float(str(GOLD['label_text']).split('\n')[2].split(' ')[3]) > np.pi       # the alpha > pi branch is in the file


# ------------------------------------------------------------------------------------------------------------ the line rule
def _fixture_lines():
    off = GOLD['line_offsets']
    for i, ((h, w), seg) in enumerate(zip(GOLD['line_shapes'], GOLD['line_segments'])):
        pil = np.unpackbits(GOLD['line_pixels'][off[i]:off[i + 1]])[:h * w].reshape(h, w).astype(bool)
        yield int(h), int(w), (int(seg[0]), int(seg[1])), (int(seg[2]), int(seg[3])), pil


def test_pillow_pixels_are_covered_and_the_rule_stays_within_its_dilation():
    n = inside_n = 0
    for h, w, a, b, pil in _fixture_lines():
        rule = R.covered(h, w, a, b, 1)
        assert not (pil & ~rule).any(), (h, w, a, b)
        if 0 <= a[0] < w and 0 <= b[0] < w and 0 <= a[1] < h and 0 <= b[1] < h:
            p = np.pad(pil, 1)
            dil = np.zeros_like(pil)
            for dy in range(3):
                for dx in range(3):
                    dil |= p[dy:dy + h, dx:dx + w]
            assert not (rule & ~dil).any(), (h, w, a, b)
            inside_n += 1
        n += 1
    assert n >= 300 and inside_n >= 150 and {tuple(s) for s in GOLD['line_shapes'].tolist()} == {(17, 23), (9, 31), (40, 40)}


def _camera_line(a, b, t, h=12, w=14):
    """The host twin's pixels of the horizontal integer segment a -> b at thickness t: an identity camera (Tr = [I | 0], K = I,
    every corner at depth 1) and a label box of zero width and height lying on the segment, so all its edges and diagonals are
    the segment, parts of it or its endpoints."""
    assert a[1] == b[1]
    cfg = R.config(t, False)
    label = np.array([[[(a[0] + b[0]) / 2.0, float(a[1]), 1.0, float(b[0] - a[0]), 0.0, 0.0, 0.0]]])
    calib = R.calib_block(np.hstack([np.eye(3), np.zeros((3, 1))]), np.eye(3))[None]
    out, _, _ = R.host_twin(cfg, np.zeros((1, 1, 9), np.float32), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32),
                            np.zeros(1, np.int32), calib, np.zeros((1, h, w, 3), np.uint8), label, np.ones(1, np.int32))
    return out[0].any(-1)


def test_known_answers_of_the_rule():
    """Worked out from the rule by hand.  t = 1: 4 d^2 <= 1 leaves only distance 0.  t = 2: 4 d^2 <= 4 is distance <= 1: the row
    itself with one more pixel beyond each end, and the rows above and below between the endpoints.  A zero-length segment at
    t = 3: 4 |p|^2 <= 9, |p|^2 <= 2.25: the 3 x 3 block, its corners included (|p|^2 = 2)."""
    seg = ((2, 5), (9, 5))
    want1 = {(x, 5) for x in range(2, 10)}
    want2 = {(x, 5) for x in range(1, 11)} | {(x, y) for x in range(2, 10) for y in (4, 6)}
    want3 = {(x, y) for x in range(3, 6) for y in (6, 7, 8)}
    as_set = lambda m: {(int(x), int(y)) for y, x in zip(*np.nonzero(m))}
    assert as_set(R.covered(12, 14, *seg, 1)) == want1
    assert as_set(R.covered(12, 14, *seg, 2)) == want2
    assert as_set(R.covered(12, 14, (4, 7), (4, 7), 3)) == want3
    # the host twin, through a flat box lying on the segment
    assert as_set(_camera_line(*seg, 1)) == want1 and as_set(_camera_line(*seg, 2)) == want2
    assert as_set(_camera_line((4, 7), (4, 7), 3)) == want3
    # a 45 degree diagonal at t = 1 is its exact pixels: off the line |cr| >= |dx| = 6, and 4 * 36 > L2 = 72
    assert as_set(R.covered(12, 14, (3, 1), (9, 7), 1)) == {(3 + k, 1 + k) for k in range(7)}
