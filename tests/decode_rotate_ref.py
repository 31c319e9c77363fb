"""TEST INFRASTRUCTURE ONLY.  numpy float64 restatement of the ``nms_type='rotate'`` branch of mmdet3d 0.18.1
``CenterHead.get_bboxes`` (``get_task_detections`` + the rotated-box BEV NMS), as DESIGN.md "Box decode: nms_type='rotate'"
defines it for this build.

PARITY UNPINNED: mmdet3d is neither vendored in the reference nor installed; nothing here was compared with upstream.
The candidates come from ``oracle.decode_ref.decode_task`` unmodified (called so that its circle NMS suppresses nothing).
The geometry is written on absolute float64 coordinates with a general convex clip; the kernel works in float32 relative
to one box's centre.  Also here: the inputs and the margin helper the CPU and the GPU test files share.
"""
import ctypes
import functools
import math

import numpy as np

from oracle import decode_ref


# ------------------------------------------------------------------------------------------------ geometry
def corners(b5):
    """(x, y, d0, d1, yaw) -> [4, 2] float64 corners: offset (ox, oy) -> (ox cos + oy sin, -ox sin + oy cos)."""
    x, y, d0, d1, yaw = (float(v) for v in b5)
    c, s = math.cos(yaw), math.sin(yaw)
    out = []
    for ox, oy in ((-d0 / 2, -d1 / 2), (-d0 / 2, d1 / 2), (d0 / 2, d1 / 2), (d0 / 2, -d1 / 2)):
        out.append((x + ox * c + oy * s, y - ox * s + oy * c))
    return np.asarray(out, np.float64)


def _signed_area(poly):
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def clip_convex(subject, clip):
    """Sutherland-Hodgman: convex ``subject`` cut by convex ``clip`` (either orientation) -> [m, 2]."""
    clip = np.asarray(clip, np.float64)
    if _signed_area(clip) < 0:
        clip = clip[::-1]                        # counter-clockwise: inside is to the left of every edge
    out = [tuple(p) for p in np.asarray(subject, np.float64)]
    for k in range(len(clip)):
        a, b = clip[k], clip[(k + 1) % len(clip)]
        side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        src, out = out, []
        for n, cur in enumerate(src):
            prev = src[n - 1]
            sp, sc = side(prev), side(cur)
            if (sp >= 0) != (sc >= 0):
                t = sp / (sp - sc)
                out.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
            if sc >= 0:
                out.append(cur)
        if not out:
            break
    return np.asarray(out, np.float64).reshape(-1, 2)


def degenerate(b5):
    x, y, d0, d1, yaw = (float(v) for v in b5)
    return not (all(math.isfinite(v) for v in (x, y, d0, d1, yaw)) and d0 > 0 and d1 > 0)


def intersection(a5, b5):
    poly = clip_convex(corners(b5), corners(a5))
    return abs(_signed_area(poly)) if len(poly) >= 3 else 0.0


def bev_iou(a5, b5):
    """IoU = inter / max(area_a + area_b - inter, 1e-8); 0 when either box is degenerate."""
    if degenerate(a5) or degenerate(b5):
        return 0.0
    a5, b5 = [float(v) for v in a5], [float(v) for v in b5]
    if math.hypot(a5[0] - b5[0], a5[1] - b5[1]) > 0.5 * (math.hypot(a5[2], a5[3]) + math.hypot(b5[2], b5[3])):
        return 0.0                               # the circumscribed circles are apart
    inter = intersection(a5, b5)
    return inter / max(a5[2] * a5[3] + b5[2] * b5[3] - inter, 1e-8)


BEV = [0, 1, 3, 4, 6]                            # (x, y, d0, d1, yaw) of a 9-column box


# ------------------------------------------------------------------------------------------------ the NMS
def nms_rotate(boxes, scores, nms_thr, score_threshold=0.0, pre_max_size=None, post_max_size=None, limit_range=None,
               decided=None):
    """boxes [n, >= 7], scores [n]: one task's ``valid_c`` candidates of one sample, in candidate order.  Returns the indices
    that are reported, in order.  ``decided``: a list that receives (i, j, iou) of every pair the walk evaluates (i kept, j > i
    still alive); the pairs of one i whose circumscribed circles are apart, IoU exactly 0, are recorded as ONE (i, -1, 0.0)."""
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    idx = np.arange(len(scores))
    if score_threshold is not None and score_threshold > 0:
        idx = idx[scores >= np.float32(score_threshold)]            # note >=; the coder's test is >
    if pre_max_size is not None and pre_max_size > 0:
        idx = idx[:pre_max_size]
    b5 = boxes[idx][:, BEV].astype(np.float64) if len(idx) else np.zeros((0, 5))
    dead = np.zeros(len(idx), bool)
    bad = np.asarray([degenerate(b) for b in b5], bool)
    with np.errstate(invalid='ignore'):
        rad = 0.5 * np.hypot(b5[:, 2], b5[:, 3])
        far = ~(np.hypot(b5[:, None, 0] - b5[None, :, 0], b5[:, None, 1] - b5[None, :, 1]) <= rad[:, None] + rad[None, :])
    far |= bad[:, None] | bad[None, :]                              # (bev_iou's own tests, for all pairs at once)
    keep = []
    cap = post_max_size if (post_max_size is not None and post_max_size > 0) else None
    for i in range(len(idx)):
        if dead[i]:
            continue
        if cap is not None and len(keep) >= cap:
            break
        keep.append(i)
        alive = ~dead
        alive[:i + 1] = False
        if decided is not None and (alive & far[i]).any():
            decided.append((int(idx[i]), -1, 0.0))
        for j in np.nonzero(alive & ~far[i])[0]:
            iou = bev_iou(b5[i], b5[j])
            if decided is not None:
                decided.append((int(idx[i]), int(idx[j]), iou))
            if iou > nms_thr:
                dead[j] = True
    keep = idx[np.asarray(keep, np.int64)]
    if limit_range is not None and len(limit_range):
        r = np.asarray(limit_range, np.float32)
        c = boxes[keep][:, :3]
        keep = keep[(c >= r[:3]).all(1) & (c <= r[3:]).all(1)]      # (after the NMS: an outside box has suppressed already)
    return keep


def task_thresholds(test_cfg, T):
    thr = test_cfg['nms_thr']
    return [float(v) for v in thr] if isinstance(thr, (list, tuple)) else [float(thr)] * T


def candidates(preds, bbox_coder, test_cfg, norm_bbox=True):
    """[task][sample] -> dict(bboxes, scores, labels): every ``valid_c`` candidate in order, through the oracle's decode_task
    with a circle NMS that suppresses nothing."""
    T = len(preds)
    open_cfg = dict(test_cfg, min_radius=[-1.0] * T, post_max_size=1 << 30)
    return [decode_ref.decode_task(p[0], bbox_coder, open_cfg, t, norm_bbox) for t, p in enumerate(preds)]


def get_bboxes_rotate(preds, bbox_coder, test_cfg, num_classes, norm_bbox=True, decided=None):
    """As ``oracle.decode_ref.get_bboxes`` with ``nms_type='rotate'``; ``decided`` collects the decided pairs' IoU and the
    task's threshold as (iou, nms_thr)."""
    T = len(preds)
    cands = candidates(preds, bbox_coder, test_cfg, norm_bbox)
    thr = task_thresholds(test_cfg, T)
    B = len(cands[0])
    out = []
    for b in range(B):
        bb, ss, ll, flag = [], [], [], 0
        for t in range(T):
            c = cands[t][b]
            pairs = [] if decided is not None else None
            keep = nms_rotate(c['bboxes'], c['scores'], thr[t], test_cfg.get('score_threshold', 0.0), test_cfg.get('pre_max_size'),
                              test_cfg.get('post_max_size'), test_cfg.get('post_center_limit_range'), pairs)
            if decided is not None:
                decided.extend((iou, thr[t]) for _, _, iou in pairs)
            box = c['bboxes'][keep].copy()
            box[:, 2] = box[:, 2] - box[:, 5] * np.float32(0.5)
            bb.append(box); ss.append(c['scores'][keep]); ll.append(c['labels'][keep] + flag)
            flag += num_classes[t]
        out.append([np.concatenate(bb), np.concatenate(ss), np.concatenate(ll).astype(np.int32)])
    return out


# ------------------------------------------------------------------------------------------------ shared test inputs
CASES = [(256, 256, 2, 500, 256), (64, 96, 1, 500, 64), (128, 128, 2, 600, 128), (512, 512, 1, 500, 512)]   # H, W, B, max_num, seed


def fake_preds(B, H, W, seed, n_obj=40):
    """The generator of tests/test_decode_gpu.py: head-like maps, low background heat with Gaussian blobs."""
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


def case_config(max_num):
    from sgv3d_amd import synthetic as S
    _, hc = S.r50_256_conf()
    hc['bbox_coder'] = dict(hc['bbox_coder'], max_num=max_num)
    hc['test_cfg'] = dict(hc['test_cfg'], nms_type='rotate')
    return hc


def host_iou(lib, a5, b5):
    """sgv3d_rotated_bev_iou_host on [n, 5] arrays -> float32 [n]."""
    a = np.ascontiguousarray(a5, np.float32).reshape(-1, 5)
    b = np.ascontiguousarray(b5, np.float32).reshape(-1, 5)
    out = np.empty(len(a), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib.sgv3d_rotated_bev_iou_host(len(a), a.ctypes.data_as(fp), b.ctypes.data_as(fp), out.ctypes.data_as(fp))
    assert rc == 0, lib.sgv3d_last_error()
    return out


def overlapping_pairs(b5):
    """(i, j), i < j, of the rows of b5 [n, 5] whose circumscribed circles meet."""
    b5 = np.asarray(b5, np.float64)
    rad = 0.5 * np.hypot(b5[:, 2], b5[:, 3])
    d = np.hypot(b5[:, None, 0] - b5[None, :, 0], b5[:, None, 1] - b5[None, :, 1])
    with np.errstate(invalid='ignore'):
        i, j = np.nonzero(np.triu(d <= rad[:, None] + rad[None, :], 1))
    return i, j


@functools.lru_cache(maxsize=None)
def host_deviation(case):
    """Largest |host float32 IoU - float64 IoU| over every overlapping candidate pair of one of CASES, and the pair count."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    H, W, B, max_num, seed = case
    hc = case_config(max_num)
    buf, layout = fake_preds(B, H, W, seed)
    preds = tuple([{k: buf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)
    worst, count = 0.0, 0
    for per_task in candidates(preds, hc['bbox_coder'], hc['test_cfg']):
        for c in per_task:
            b5 = c['bboxes'][:, BEV]
            i, j = overlapping_pairs(b5)
            if not len(i):
                continue
            got = host_iou(lib, b5[i], b5[j])
            want = np.asarray([bev_iou(b5[p], b5[q]) for p, q in zip(i, j)])
            worst = max(worst, float(np.abs(got - want).max()))
            count += len(i)
    return worst, count


def margin():
    """m = 8 x the largest deviation of the host build of the kernel's float32 geometry from the float64 reference over the
    overlapping candidate pairs of all CASES: how close to nms_thr a decided pair's IoU may be before float32 may decide it
    the other way."""
    devs = [host_deviation(c) for c in CASES]
    m = 8.0 * max(d for d, _ in devs)
    print("rotate NMS margin: deviations", ["%.3g over %d pairs" % d for d in devs], "-> m = %.3g" % m)
    return m
