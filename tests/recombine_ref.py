"""Float64 numpy restatement of SGV3D's frame recombination (the reference's scripts/data_preprocess/recombine_utils.py:
``get_M``, ``transform_with_M_bilinear``, ``unify_extrinsic_params_tools``, ``update_bbox_info``, ``iou``,
``objects_combine_tools``, ``label_generation``), the yardstick of csrc/recombine.hip.

Every per-pixel and per-object expression is written out elementwise in the reference's operation order (no
``np.matmul`` on the per-pixel product: a BLAS may fuse).  Frames are uint8 RGB (the reference's are BGR: channel 2 is B
here).  Two OpenCV rules are restated without cv2 at hand, as in train_augment_ref.py: the 8-bit fixed-point gray of
``cvtColor`` (float path: ``0.114 B + 0.587 G + 0.299 R`` in float32) and ``convertScaleAbs`` (``|x + beta|`` in
float32, ties to even, saturated).  SAM is replaced by the stated stand-in: the source's stored class-id mask, sampled at
the warp position (nearest neighbour) and kept inside the union of the source's accepted boxes.

A frame is a dict: ``image`` u8 [H, W, 3], ``mask`` u8 [H, W], ``Tr_ego2cam`` [4, 4], ``P2`` [3, 4] and ``objects``, a
dict of ``corners`` f64 [n, 3, 8] (ego frame), ``dim`` [n, 3] (h, w, l), ``truncated``, ``occluded``, ``score`` [n] and
``names`` (n strings).  Source objects are already filtered as ``load_annos`` does and in the order of the random draw.
"""
import math

import numpy as np

FOCUS = ("car", "van", "truck", "bus", "pedestrian", "cyclist")
NAMES = FOCUS + ("bicycle", "tricyclist", "motorcycle", "motorcyclist")


# ------------------------------------------------------------------------------------------------------------------ warp
def homography(Tr_src, P2_src, Tr_dest, P2_dest):
    """``get_M`` on the 3x3 blocks: M = K_d R_d R_s^-1 K_s^-1; returns (M, inv(M)).  The products are float64; a float32
    P2 (what the reference's calib loader returns) is inverted by numpy in float32 first, as the reference inverts it."""
    R, K = np.asarray(Tr_src)[:3, :3], np.asarray(P2_src)[:3, :3]          # the arrays' own dtypes: see the docstring
    R_r, K_r = np.asarray(Tr_dest)[:3, :3], np.asarray(P2_dest)[:3, :3]
    M = np.matmul(np.matmul(np.matmul(K_r, R_r), np.linalg.inv(R)), np.linalg.inv(K))
    return M, np.linalg.inv(M)


def warp_positions(Minv, H, W):
    """-> (qx, qy, dead): the clipped source position of every destination pixel and the dead flag."""
    m = np.asarray(Minv, np.float64).reshape(9)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y, z = u * 10.0, v * 10.0, 10.0
    px = (m[0] * x + m[1] * y) + m[2] * z
    py = (m[3] * x + m[4] * y) + m[5] * z
    pz = (m[6] * x + m[7] * y) + m[8] * z
    with np.errstate(all='ignore'):
        qx, qy = px / pz, py / pz
    bad = ~(np.isfinite(qx) & np.isfinite(qy))                   # the reference would fail on its index: dead here
    qx, qy = np.where(bad, 0.0, qx), np.where(bad, 0.0, qy)
    dead = bad | (qx < 0) | (qx > W - 2) | (qy < 0) | (qy > H - 2)
    return np.clip(qx, 0, W - 2), np.clip(qy, 0, H - 2), dead


def warp_bilinear(image, Minv):
    """``transform_with_M_bilinear`` -> float32 [H, W, 3]."""
    H, W = image.shape[:2]
    qx, qy, dead = warp_positions(Minv, H, W)
    c0, r0 = np.floor(qx).astype(np.int32), np.floor(qy).astype(np.int32)
    img = image.astype(np.float64)
    wl, wr = ((c0 + 1) - qx)[..., None], (qx - c0)[..., None]
    fr1 = wl * img[r0, c0] + wr * img[r0, c0 + 1]
    fr2 = wl * img[r0 + 1, c0] + wr * img[r0 + 1, c0 + 1]
    out = ((r0 + 1) - qy)[..., None] * fr1 + (qy - r0)[..., None] * fr2
    out[dead] = 0.0
    return out.astype(np.float32)


def warp_nearest(mask, Minv):
    """The stand-in's class ids: the stored mask at floor(q + 0.5), 0 where dead, clipped to 0..6."""
    H, W = mask.shape
    qx, qy, dead = warp_positions(Minv, H, W)
    out = np.minimum(mask[np.floor(qy + 0.5).astype(np.int32), np.floor(qx + 0.5).astype(np.int32)], 6)
    out[dead] = 0
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ brightness
def gray_u8(rgb):
    v = rgb.astype(np.int64)
    return ((v[..., 2] * 1868 + v[..., 1] * 9617 + v[..., 0] * 4899 + 8192) >> 14).astype(np.uint8)


def gray_f32(rgb):
    v = rgb.astype(np.float32)
    return (np.float32(0.114) * v[..., 2] + np.float32(0.587) * v[..., 1]) + np.float32(0.299) * v[..., 0]


def beta_of(bd, bs):
    with np.errstate(all='ignore'):
        beta = float(100 * (np.float64(bd) - np.float64(bs)) / np.float64(bs))
    return (1 if beta > 0 else -1) * min(abs(beta), 60)


def shift_abs(img32, beta):
    """-> (uint8 result, |x + beta| in float32): ``convertScaleAbs(img, alpha=1, beta=beta)``."""
    t = np.abs(img32.astype(np.float32) + np.float32(beta))
    with np.errstate(invalid='ignore'):
        r = np.rint(t)
    return np.where(r > 0, np.minimum(r, 255), 0).astype(np.uint8), t


# ----------------------------------------------------------------------------------------------------------------- boxes
def camera_corners(corners, delta, Tr):
    """[3, 8] ego corners (+ delta) through Tr_ego2cam -> [8, 3] camera-frame corners."""
    c = np.asarray(corners, np.float64)
    if delta is not None:
        c = c + np.asarray(delta, np.float64)[:, None]
    t = np.asarray(Tr, np.float64)
    return np.stack([((t[r, 0] * c[0] + t[r, 1] * c[1]) + t[r, 2] * c[2]) + t[r, 3] for r in range(3)], 1)


def float_box(corners, delta, Tr, P2):
    """``update_bbox_info`` -> ([xmin, ymin, xmax, ymax] as the reference holds them, an int 0 where clamped) or None."""
    c = camera_corners(corners, delta, Tr)
    p = np.asarray(P2, np.float64)
    h = [((p[r, 0] * c[:, 0] + p[r, 1] * c[:, 1]) + p[r, 2] * c[:, 2]) + p[r, 3] for r in range(3)]
    with np.errstate(all='ignore'):
        u, v = h[0] / h[2], h[1] / h[2]
    xmin, ymin, xmax, ymax = np.min(u), np.min(v), np.max(u), np.max(v)
    if xmax <= 0 or ymax <= 0:
        return None
    return [max(0, xmin), max(0, ymin), xmax, ymax]


def int_box(box, H, W):
    with np.errstate(invalid='ignore'):
        xmin, ymin, xmax, ymax = (int(v) for v in np.array(box, np.float64).astype(np.int32))
    if xmax <= 0 or ymax <= 0:
        return None
    xmin, ymin = max(0, xmin), max(0, ymin)
    xmax, ymax = min(xmax, W - 1), min(ymax, H - 1)
    if xmax <= xmin or ymax <= ymin or xmax - xmin <= 1 or ymax - ymin <= 1:
        return None
    return [xmin, ymin, xmax, ymax]


def iou(boxes, box):
    """``iou(boxes, box[None])[:, 0]``: intersection over (area + area - intersection + 10e-9)."""
    a, b = np.asarray(boxes, np.float64), np.asarray(box, np.float64)
    ih = np.maximum(0.0, np.minimum(a[:, 2], b[2]) - np.maximum(a[:, 0], b[0]))
    iw = np.maximum(0.0, np.minimum(a[:, 3], b[3]) - np.maximum(a[:, 1], b[1]))
    inter = ih * iw
    union = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter
    return inter / (union + 10e-9)


def gate(init_boxes, candidates, thr=0.15):
    """``candidates``: int boxes or None, in walk order -> (kept flags, the grown list)."""
    acc = [list(b) for b in init_boxes] or [[0, 0, 0, 0]]
    kept = []
    for box in candidates:
        ok = box is not None and bool(np.max(iou(acc, box)) < thr)
        if ok:
            acc.append(list(box))
        kept.append(ok)
    return kept, acc


# ---------------------------------------------------------------------------------------------------------------- labels
def label_fields(corners, delta, Tr, dim, bbox, score):
    """``label_generation`` -> the unrounded alpha, bbox, h, w, l, location, rotation_y, score."""
    c = camera_corners(corners, delta, Tr)
    s = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]))       # np.mean's pairwise tree over eight rows
    loc = s / 8.0
    h, w, l = (float(v) for v in dim)
    loc[1] = loc[1] + h / 2
    dx, dz = c[0, 0] - c[3, 0], c[0, 2] - c[3, 2]
    rotation = math.atan2(-dz, dx)
    alpha = rotation - math.atan2(loc[0], loc[2])
    if alpha > math.pi:
        alpha = alpha - 2.0 * math.pi
    if alpha <= (-1 * math.pi):
        alpha = alpha + 2.0 * math.pi
    at = math.atan(math.tan(alpha))
    alpha = at + math.pi if math.cos(alpha) < 0 else at
    return [alpha] + list(bbox) + [h, w, l, float(loc[0]), float(loc[1]), float(loc[2]), rotation, float(score)]


def label_line(name, truncated, occluded, fields):
    """One line of the label file: Python's ``round(v, 4)`` and ``str``; a clamped minimum is the integer 0."""
    return " ".join([name, str(float(truncated)), str(float(occluded))] +
                    [str(round(v, 4)) if isinstance(v, int) else repr(round(float(v), 4)) for v in fields])


# -------------------------------------------------------------------------------------------------------------- pipeline
def recombine(dest, sources):
    """One generated frame -> dict(image, mask, beta [S], boxes (float box or None per object, the destination's first),
    kept (flag per object), lines (label text), warped [S] float32, shifted_abs [S] the float32 |x + beta|)."""
    H, W = dest['image'].shape[:2]
    Tr, P2 = np.asarray(dest['Tr_ego2cam'], np.float64), np.asarray(dest['P2'], np.float64)
    out_img, out_mask = dest['image'].copy(), np.minimum(dest['mask'], 6).astype(np.uint8)
    bd = np.mean(gray_u8(dest['image']))
    boxes, kept, lines, betas, warped_all, abs_all = [], [], [], [], [], []

    def emit(o, i, delta, box):
        f = label_fields(o['corners'][i], delta, Tr, o['dim'][i], box, o['score'][i])
        lines.append(label_line(o['names'][i], o['truncated'][i], o['occluded'][i], f))

    o = dest['objects']
    acc = []
    for i in range(len(o['names'])):
        box = float_box(o['corners'][i], None, Tr, P2)
        boxes.append(box)
        kept.append(box is not None)
        if box is not None:
            acc.append(box)
            emit(o, i, None, box)
    acc = acc or [[0, 0, 0, 0]]
    for src in sources:
        _, Minv = homography(src['Tr_ego2cam'], src['P2'], Tr, P2)
        delta = np.linalg.inv(Tr)[:3, 3] - np.linalg.inv(np.asarray(src['Tr_ego2cam'], np.float64))[:3, 3]
        warped = warp_bilinear(src['image'], Minv)
        bs = np.sum(gray_f32(warped).astype(np.float64)) / (H * W)
        beta = beta_of(bd, bs)
        shifted, t = shift_abs(warped, beta)
        o = src['objects']
        inside = np.zeros((H, W), bool)
        for i in range(len(o['names'])):
            box = float_box(o['corners'][i], delta, Tr, P2)
            boxes.append(box)
            ib = int_box(box, H, W) if box is not None and o['names'][i].lower() in FOCUS else None
            ok = ib is not None and bool(np.max(iou(acc, ib)) < 0.15)
            kept.append(ok)
            if ok:
                acc.append(ib)
                inside[ib[1]:ib[3] + 1, ib[0]:ib[2] + 1] = True
                emit(o, i, delta, box)
        ids = np.where(inside, warp_nearest(src['mask'], Minv), 0).astype(np.uint8)
        on = ids > 0
        out_img = np.where(on[..., None], shifted, out_img)
        out_mask = np.clip(np.where(on, ids, out_mask), 0, 6).astype(np.uint8)
        betas.append(beta), warped_all.append(warped), abs_all.append(t)
    return dict(image=out_img, mask=out_mask, beta=betas, boxes=boxes, kept=kept, lines=lines, warped=warped_all,
                shifted_abs=abs_all, accepted=acc)
