"""The renderer's contract (DESIGN.md "Rendering detections") restated in numpy / Python: float64 geometry one rounding at a time,
int64 coverage, order by painting the primitives in ascending number.  Written from the rules, not from csrc/render.hip.  Also
the scenes the CPU and GPU tests share, and the ctypes call of the host twin."""
import ctypes
import math

import numpy as np

from sgv3d_amd import _lib
from sgv3d_amd.evaluators.device_kitti import calib_block, class_table
from sgv3d_amd.evaluators.result2kitti import category_map_dair

GUARD = 64.0
EOVERFLOW = 1
CAM_EDGES = [(0, 1), (1, 5), (5, 4), (4, 0), (1, 2), (2, 6), (6, 5), (2, 3), (3, 7), (7, 6), (3, 0), (4, 7)]   # faces 0..3, duplicates left out
CAM_DIAGONALS = [(0, 5), (1, 4)]
BEV_EDGES = [(0, 1), (0, 3), (1, 2), (2, 3)]
F = np.float64


# ------------------------------------------------------------------------------------------------------------ coverage
def covered(h, w, a, b, t):
    """bool [h, w]: the pixels of an h x w target the segment a -> b covers at thickness t (integers throughout)."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    ax, ay, bx, by = (int(v) for v in (*a, *b))
    dx, dy = bx - ax, by - ay
    px, py = xs - ax, ys - ay
    L2 = dx * dx + dy * dy
    s = px * dx + py * dy
    cr = px * dy - py * dx
    t2 = t * t
    near_a = 4 * (px * px + py * py) <= t2
    near_b = 4 * ((xs - bx) ** 2 + (ys - by) ** 2) <= t2
    if L2 == 0:
        return near_a
    return np.where(s <= 0, near_a, np.where(s >= L2, near_b, 4 * cr * cr <= t2 * L2))


def paint(img, prims):
    """prims: [(x0, y0, x1, y1, t, rgb)] in ascending number; the last one covering a pixel owns it."""
    h, w = img.shape[:2]
    for x0, y0, x1, y1, t, rgb in prims:
        g = (t + 1) // 2
        lo_x, hi_x = max(0, min(x0, x1) - g), min(w - 1, max(x0, x1) + g)
        lo_y, hi_y = max(0, min(y0, y1) - g), min(h - 1, max(y0, y1) + g)
        if lo_x > hi_x or lo_y > hi_y:
            continue
        m = covered(hi_y - lo_y + 1, hi_x - lo_x + 1, (x0 - lo_x, y0 - lo_y), (x1 - lo_x, y1 - lo_y), t)
        img[lo_y:hi_y + 1, lo_x:hi_x + 1][m] = rgb


# ------------------------------------------------------------------------------------------------------------ geometry
def dot3(m, a, b, c):
    return (m[0] * a + m[1] * b) + m[2] * c


def _cos(v):
    return F(math.cos(v)) if math.isfinite(v) else F('nan')


def _sin(v):
    return F(math.sin(v)) if math.isfinite(v) else F('nan')


def box_corner(k, ex, ey, h, c, s, x, y, z):
    hx, hy = ex / F(2), ey / F(2)
    lx = -hx if k & 2 else hx
    ly = -hy if (k + 1) & 2 else hy
    lz = h if k & 4 else F(0)
    return [(c * lx + (-s) * ly) + x, (s * lx + c * ly) + y, lz + z]


def pred_corners(box, cal):
    Rm, tr = cal[21:30], cal[30:33]
    bx, by, bz = (F(v) for v in box[:3])
    x = dot3(Rm[0:3], bx, by, bz) + tr[0]
    y = dot3(Rm[3:6], bx, by, bz) + tr[1]
    z = dot3(Rm[6:9], bx, by, bz) + tr[2]
    w, l, h, yaw = F(box[4]), F(box[3]), F(box[5]), F(box[6])
    zb = (z + h / F(2)) - h / F(2)
    return [box_corner(k, w, l, h, _cos(yaw), _sin(yaw), x, y, zb) for k in range(8)]


def label_corners(row):
    r = [F(v) for v in row]
    return [box_corner(k, r[3], r[4], r[5], _cos(r[6]), _sin(r[6]), r[0], r[1], r[2]) for k in range(8)]


def clip(a, b, w, h):
    """Liang-Barsky against the guard rectangle, borders left, right, top, bottom; -> integer endpoints or None."""
    ax, ay, bx, by = a[0], a[1], b[0], b[1]
    if not all(math.isfinite(v) for v in (ax, ay, bx, by)):
        return None
    dx, dy = bx - ax, by - ay
    if not (math.isfinite(dx) and math.isfinite(dy)):
        return None
    t0, t1 = F(0), F(1)
    for p, q in ((-dx, ax - (-GUARD)), (dx, (F(w) + GUARD) - ax), (-dy, ay - (-GUARD)), (dy, (F(h) + GUARD) - ay)):
        if p == 0:
            if q < 0:
                return None
            continue
        r = q / p
        if p < 0:
            if r > t1:
                return None
            if r > t0:
                t0 = r
        else:
            if r < t0:
                return None
            if r < t1:
                t1 = r
    x0, y0 = (ax + t0 * dx, ay + t0 * dy) if t0 > 0 else (ax, ay)
    x1, y1 = (ax + t1 * dx, ay + t1 * dy) if t1 < 1 else (bx, by)
    return int(x0), int(y0), int(x1), int(y1)


def camera_prims(P, cal, w, h, z_near, thickness, rgb):
    Tr, K = cal[:12], cal[12:21]
    H = [[dot3(Tr[0:3], *p) + Tr[3], dot3(Tr[4:7], *p) + Tr[7], dot3(Tr[8:11], *p) + Tr[11]] for p in P]

    def project(c):
        d = dot3(K[6:9], *c)
        return dot3(K[0:3], *c) / d, dot3(K[3:6], *c) / d

    out = []
    zn = F(z_near)
    for e, (i, j) in enumerate(CAM_EDGES + CAM_DIAGONALS):
        a, b = list(H[i]), list(H[j])
        a_behind, b_behind = bool(a[2] < zn), bool(b[2] < zn)
        if a_behind and b_behind:
            continue
        if a_behind:
            s = (zn - a[2]) / (b[2] - a[2])
            a = [a[k] + s * (b[k] - a[k]) for k in range(3)]
        elif b_behind:
            s = (zn - b[2]) / (a[2] - b[2])
            b = [b[k] + s * (a[k] - b[k]) for k in range(3)]
        seg = clip(project(a), project(b), w, h)
        if seg is not None:
            out.append((*seg, thickness if e < 12 else 1, rgb))
    return out


def bev_points(P, res, x_off, y_off):
    """pcl2xy_plane on corners 0..3 -> [(x_img, y_img) or None]."""
    pts = []
    for k in range(4):
        vx, vy = -P[k][1] / F(res), -P[k][0] / F(res)
        if not (abs(vx) < 2147483648.0 and abs(vy) < 2147483648.0):
            pts.append(None)
            continue
        pts.append((int(vx) - x_off, int(vy) + y_off))
    return pts


def bev_prims(P, bev, rgb):
    pts = bev_points(P, bev['res'], bev['x_off'], bev['y_off'])
    out = []
    for i, j in BEV_EDGES:
        if pts[i] is None or pts[j] is None:
            continue
        seg = clip((F(pts[i][0]), F(pts[i][1])), (F(pts[j][0]), F(pts[j][1])), bev['w'], bev['h'])
        if seg is not None:
            out.append((*seg, 2, rgb))
    return out


def render(cfg, boxes, scores, labels, counts, calib, frames, label_rows=None, label_counts=None, masks=None):
    """-> (out [B, H, W, 3], bev [B, Hb, Wb, 3] or None, status [B]).  ``cfg``: see ``config``."""
    B, H, W = frames.shape[:3]
    bev_cfg = cfg['bev']
    out = frames.copy()
    bev = np.zeros((B, bev_cfg['h'], bev_cfg['w'], 3), np.uint8) if bev_cfg else None
    status = np.zeros(B, np.int32)
    table = cfg['table']
    with np.errstate(all='ignore'):
        for b in range(B):
            n = min(max(int(counts[b]), 0), boxes.shape[1])
            kept = [r for r in range(n) if F(scores[b, r]) > cfg['score_thr'] and 0 <= labels[b, r] < len(table) and table[labels[b, r]] >= 0]
            nlab = 0 if label_rows is None else min(max(int(label_counts[b]), 0), label_rows.shape[1])
            if len(kept) > cfg['max_boxes'] or nlab > cfg['max_boxes']:
                status[b] = EOVERFLOW
                continue
            cam, bv = [], []
            for r in kept:
                P = pred_corners(boxes[b, r], calib[b])
                cam += camera_prims(P, calib[b], W, H, cfg['z_near'], cfg['thickness'], cfg['class_colors'][labels[b, r]])
                if bev_cfg:
                    bv += bev_prims(P, bev_cfg, cfg['bev_pred_color'])
            for r in range(nlab):
                P = label_corners(label_rows[b, r])
                cam += camera_prims(P, calib[b], W, H, cfg['z_near'], cfg['thickness'], cfg['label_color'])
                if bev_cfg:
                    bv += bev_prims(P, bev_cfg, cfg['bev_label_color'])
            if masks is not None:
                ids = masks[b].astype(np.int64) // 40
                on = (ids >= 1) & (ids <= 6)
                pal = np.asarray(cfg['palette'], np.int64)[ids]
                mixed = (out[b].astype(np.int64) * (256 - cfg['mask_alpha']) + pal * cfg['mask_alpha'] + 128) >> 8
                out[b][on] = mixed[on].astype(np.uint8)
            paint(out[b], cam)
            if bev_cfg:
                paint(bev[b], bv)
    return out, bev, status


# ------------------------------------------------------------------------------------------------------------ configuration
CLASS_NAMES = ['car', 'truck', 'bus', 'pedestrian', 'bicycle', 'traffic_cone']        # traffic_cone is not in the category map
TABLE = class_table(CLASS_NAMES, category_map_dair)
CLASS_COLORS = [(0, 255, 0), (255, 255, 0), (255, 255, 0), (0, 255, 255), (255, 255, 255), (255, 255, 255)]
PALETTE = [(0, 0, 0), (0, 255, 0), (255, 255, 0), (0, 255, 255), (255, 0, 0), (255, 0, 255), (0, 128, 255)]
SMALL_BEV = dict(side_range=(-6, 6), fwd_range=(0, 20), res=0.25)


def bev_config(side_range, fwd_range, res):
    return dict(w=1 + int((side_range[1] - side_range[0]) / res), h=1 + int((fwd_range[1] - fwd_range[0]) / res), res=res,
                x_off=int(np.floor(side_range[0] / res)), y_off=int(np.ceil(fwd_range[1] / res)))


def config(thickness=2, bev=True, max_boxes=32, mask_alpha=96, z_near=0.5):
    return dict(thickness=thickness, bev=bev_config(**SMALL_BEV) if bev else None, max_boxes=max_boxes, mask_alpha=mask_alpha,
                z_near=z_near, score_thr=0.45, table=TABLE, class_colors=CLASS_COLORS, label_color=(255, 0, 0),
                bev_pred_color=(0, 0, 255), bev_label_color=(255, 0, 0), palette=PALETTE)


def make_desc(cfg, B, N, m, H, W, f64):
    d = _lib.RenderDesc()
    d.batch, d.n, d.m, d.height, d.width = B, N, m, H, W
    if cfg['bev']:
        bv = cfg['bev']
        d.bev_h, d.bev_w, d.bev_x_off, d.bev_y_off, d.bev_res = bv['h'], bv['w'], bv['x_off'], bv['y_off'], bv['res']
    d.max_boxes, d.thickness, d.f64_inputs, d.num_classes, d.mask_alpha = cfg['max_boxes'], cfg['thickness'], int(f64), len(cfg['table']), cfg['mask_alpha']
    d.score_thr, d.z_near = cfg['score_thr'], cfg['z_near']
    for k in range(64):
        d.class_table[k] = int(cfg['table'][k]) if k < len(cfg['table']) else -1
    for name in ('class_colors', 'label_color', 'bev_pred_color', 'bev_label_color', 'palette'):
        flat = np.asarray(cfg[name]).reshape(-1)
        arr = getattr(d, name)
        for k, v in enumerate(flat):
            arr[k] = int(v)
    return d


def host_twin(cfg, boxes, scores, labels, counts, calib, frames, label_rows=None, label_counts=None, masks=None, in_place=False):
    """sgv3d_render_detections_host over numpy arrays -> (out, bev, status)."""
    B, H, W = frames.shape[:3]
    boxes, scores = np.ascontiguousarray(boxes), np.ascontiguousarray(scores)
    f64 = boxes.dtype == np.float64
    assert scores.dtype == boxes.dtype and labels.dtype == np.int32 and counts.dtype == np.int32 and calib.dtype == np.float64
    m = 0 if label_rows is None else label_rows.shape[1]
    d = make_desc(cfg, B, boxes.shape[1], m, H, W, f64)
    out = frames.copy() if in_place else np.full_like(frames, 0xA5)
    src = out if in_place else np.ascontiguousarray(frames)
    bev = np.full((B, cfg['bev']['h'], cfg['bev']['w'], 3), 0xA5, np.uint8) if cfg['bev'] else None
    status = np.full(B, -9, np.int32)
    P = lambda a: None if a is None else a.ctypes.data
    rc = _lib.load().sgv3d_render_detections_host(ctypes.byref(d), P(boxes), P(scores), P(labels), P(counts), P(calib), P(label_rows),
                                                  P(label_counts), P(src), P(masks), P(out), P(bev), P(status))
    _lib.check(rc, "sgv3d_render_detections_host")
    return out, bev, status


# ------------------------------------------------------------------------------------------------------------ scenes
def scene_calib(H, W, B):
    """A camera 1.5 m up looking along lidar +x with a slight pitch and roll; 90 degree horizontal field of view."""
    blocks = []
    for b in range(B):
        pitch, roll = 0.06 + 0.01 * b, 0.013 * b
        base = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
        cp, sp, cr, sr = math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
        Rp = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        Rr = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
        Tr = np.zeros((3, 4))
        Tr[:, :3] = Rr @ Rp @ base
        Tr[:, 3] = [0.03, 1.5, 0.11]
        K = np.array([[W / 2 + 0.37, 0.0, W / 2 - 0.21], [0.0, W / 2 + 0.11, H / 2 + 0.4], [0.0, 0.0, 1.0]])
        blocks.append(calib_block(Tr, K, (1.0, 0.0, 0.0, 0.01 * b), (0.1 * b, -0.05 * b, 0.0)))
    return np.stack(blocks)


# x, y, z, l, w, h, yaw, vx, vy | score | class: the cases of the GPU tests, hand-placed for the camera above
SCENE_ROWS = [
    ([12.0, 0.3, 0.0, 4.2, 1.9, 1.6, 0.3, 0, 0], 0.9, 0),             # wholly in view
    ([10.0, 10.2, 0.0, 4.0, 2.0, 1.5, 0.1, 0, 0], 0.8, 1),            # straddles the left edge
    ([10.0, -10.1, 0.0, 4.0, 2.0, 1.5, -0.2, 0, 0], 0.8, 2),          # straddles the right edge
    ([8.0, 1.0, 6.3, 3.0, 2.0, 2.5, 0.7, 0, 0], 0.7, 0),              # straddles the top edge
    ([6.0, -1.0, -2.6, 3.0, 2.0, 2.0, 1.1, 0, 0], 0.7, 3),            # straddles the bottom edge
    ([1.2, 0.4, 0.2, 4.0, 1.8, 1.4, 0.05, 0, 0], 0.95, 0),            # straddles the near plane
    ([-10.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0, 0, 0], 0.9, 0),            # wholly behind the camera
    ([5.0, 700.0, 0.0, 4.0, 2.0, 1.5, 0.0, 0, 0], 0.9, 1),            # far outside the guard rectangle
    ([15.0, 2.0, 0.5, 0.0, 0.0, 0.0, 0.4, 0, 0], 0.9, 4),             # zero extents
    ([float('nan'), 1.0, 0.0, 4.0, 2.0, 1.5, 0.2, 0, 0], 0.9, 0),     # a NaN row
    ([14.0, -2.0, 0.0, 4.0, 2.0, 1.5, 0.2, 0, 0], 0.45, 0),           # the score threshold exactly: not kept
    ([13.0, 3.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0, 0], 0.9, 5),             # an unmapped class
    ([16.0, -3.0, 0.0, 4.5, 2.0, 1.7, 0.5, 0, 0], 0.6, 0),            # two overlapping boxes of different classes:
    ([16.5, -2.6, 0.1, 9.0, 2.6, 3.2, 0.45, 0, 0], 0.6, 2),           # the later one wins where both cover a pixel
    ([18.0, 4.0, 0.0, 0.8, 0.7, 1.8, 0.0, 0, 0], 0.46, 3),
    ([12.0, 0.3, 0.0, 4.2, 1.9, 1.6, float('inf'), 0, 0], 0.9, 0),    # an infinite yaw
    ([0.9, 0.0, 0.0, 0.0, 0.2, 1.0, 0.0, 0, 0], 0.9, 1),              # scene() makes it so long that u is near -+1.5e308 (float64 rows)
]
LABEL_ROWS = [[12.2, 0.2, 0.05, 4.0, 1.8, 1.5, 0.28], [16.2, -2.9, 0.0, 4.4, 2.1, 1.6, 0.52], [9.0, 30.0, 0.0, 4.0, 2.0, 1.5, 1.0]]


def scene(H, W, B, dtype=np.float32, seed=0, labels=True, pad=3):
    """The hand-placed rows in every sample, shifted a little per sample, plus ``pad`` rows beyond counts[b] that must not be
    read as detections."""
    rng = np.random.default_rng(seed + 1000 * B + H)
    n = len(SCENE_ROWS)
    boxes = np.zeros((B, n + pad, 9), dtype)
    scores = np.zeros((B, n + pad), dtype)
    cls = np.zeros((B, n + pad), np.int32)
    for b in range(B):
        for r, (row, sc, c) in enumerate(SCENE_ROWS):
            boxes[b, r] = row
            boxes[b, r, 0] += 0.37 * b
            boxes[b, r, 6] += 0.21 * b
            scores[b, r], cls[b, r] = sc, c
        # at depth 1 the two ends project near -+1.5e308: finite, their difference is not (sample 0; the others stay finite)
        boxes[b, n - 1, 3] = dtype(2.0) * (dtype(1.6e308) / dtype(W / 2 + 0.37)) if dtype is np.float64 else 3.0e38
        boxes[b, n:, :7] = [11.0, 0.0, 0.0, 3.0, 2.0, 1.5, 0.0]        # beyond the count: would be drawn if read
        scores[b, n:], cls[b, n:] = 0.99, 0
    counts = np.full(B, n, np.int32)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    masks = (rng.integers(0, 7, (B, H // 8 + 1, W // 8 + 1)).repeat(8, 1).repeat(8, 2)[:, :H, :W] * 40).astype(np.uint8)
    masks[:, ::5, ::7] = rng.integers(0, 256, masks[:, ::5, ::7].shape, dtype=np.uint8)       # values that are no multiple of 40
    lab = lc = None
    if labels:
        lab = np.zeros((B, len(LABEL_ROWS) + 1, 7))
        lab[:, :len(LABEL_ROWS)] = LABEL_ROWS
        lab[:, len(LABEL_ROWS)] = [11.0, 0.0, 0.0, 3.0, 2.0, 1.5, 0.0]  # beyond the label count
        lc = np.full(B, len(LABEL_ROWS), np.int32)
        if B > 1:
            lc[1] = 1
    return dict(boxes=boxes, scores=scores, labels=cls, counts=counts, calib=scene_calib(H, W, B), frames=frames, masks=masks,
                label_rows=lab, label_counts=lc)


SIZES = [(40, 64), (37, 61), (130, 260)]
BATCHES = [1, 3]


def variants():
    """(thickness, bev, masks, in_place) of every GPU-test case."""
    return [(t, bev, mk, ip) for t in (1, 2, 3) for bev in (False, True) for mk in (False, True) for ip in (False, True)]


# The scenes only single GPU tests use; the CPU file runs them through the restatement too.
def scene_empty_sample():
    sc = scene(37, 61, 3)
    sc['counts'][1] = 0
    return sc


def scene_constant():
    sc = scene(130, 260, 3)
    sc['frames'][:] = 0x5B
    return sc


def scene_replay():
    sc = scene(37, 61, 3, seed=5)
    sc['boxes'][:, :, 1] += 0.8
    sc['boxes'][:, :, 6] -= 0.3
    sc['counts'][:] = [len(SCENE_ROWS), 5, 0]
    return sc


def extra_cases():
    """(name, scene, config, masks, in_place, labels) of those tests."""
    return [("empty sample, no labels", scene_empty_sample(), config(2, True), False, False, False),
            ("constant frames in place", scene_constant(), config(2, True), False, True, True),
            ("constant frames out of place", scene_constant(), config(2, True), False, False, True),
            ("graph replay", scene_replay(), config(2, True), True, False, True)]
