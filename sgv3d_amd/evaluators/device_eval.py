"""The KITTI AP tables on the device (csrc/kitti_eval_device.hip): ``kitti_eval_device`` takes the annotation lists
``kitti_eval`` takes and returns the same ``(result text, ret_dict)``.

``kitti_eval`` walks the set on the host: ``clean_data`` per image, class and difficulty, then one
``sgv3d_kitti_eval_curves`` call per (metric, class, difficulty, minimum overlap).  Here the annotations are packed once
into one pinned buffer (the ground-truth side can be packed ahead with ``pack_ground_truth`` and handed over in place of
the list), uploaded in one copy, and eight launches produce every cell's precision / recall / orientation curve; one copy
brings the curves and the threshold counts back.  What happens before (``eval_setup``: class names, minimum overlaps, the
``compute_aos`` rule) and after (``get_mAP*``, ``eval_report``: the AP reduction and the report text) is the code
``kitti_eval`` runs.  The host path stays as the yardstick and the default everywhere.

There is no CPU path: without a GPU ``kitti_eval_device`` raises.  ``curves_host`` runs the kernels' functions on the host
over the same packed buffer (``sgv3d_kitti_eval_device_host``); it needs the BEV / 3-D overlaps from the caller and exists
for the tests."""
import numpy as np
import torch

from .. import _lib, hip_ops
from .kitti_utils.eval import eval_report, eval_setup, get_mAP, get_mAP_R40

__all__ = ['kitti_eval_device', 'pack_ground_truth', 'pack_annotations', 'curves_host', 'name_ids', 'PackedGroundTruth',
           'MAX_DETECTIONS']

GT_FIELDS, DT_FIELDS, POINTS, TILE = 14, 13, 41, 16
MAX_DETECTIONS = 4096                    # per image: one bit per detection in a lane's 64-bit masks
_KINDS = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'bus': 3, 'van': 4, 'person_sitting': 5}
_OTHER, _DONTCARE = 6, 8
_METRIC = {'bbox': 0, 'bev': 1, '3d': 2}


def _up8(n):
    return (n + 7) // 8 * 8


def name_ids(names, dontcare=True):
    """int32 per name: what ``clean_data`` distinguishes -- the kind of the lower-cased name (0 car, 1 pedestrian, 2 cyclist,
    3 bus, 4 van, 5 person_sitting, 6 anything else) plus 8 for the exact spelling ``DontCare``."""
    out = np.empty(len(names), np.int32)
    for i, n in enumerate(names):
        n = str(n)
        out[i] = _KINDS.get(n.lower(), _OTHER) | (_DONTCARE if dontcare and n == 'DontCare' else 0)
    return out


def _f64(a, width):
    return np.asarray(a, np.float64).reshape(-1, width)


class PackedGroundTruth:
    """The ground-truth side of the packed input: rows f64 [TG, 14], name ids i32 [TG], counts per image."""

    def __init__(self, gt_annos):
        self.annos = gt_annos
        self.counts = np.array([len(g['name']) for g in gt_annos], np.int64)
        rows = [np.concatenate([_f64(g['bbox'], 4), _f64(g['alpha'], 1), _f64(g['location'], 3), _f64(g['dimensions'], 3),
                                _f64(g['rotation_y'], 1), _f64(g['truncated'], 1), _f64(g['occluded'], 1)], 1) for g in gt_annos]
        self.rows = np.concatenate(rows, 0) if rows else np.zeros((0, GT_FIELDS))
        self.names = np.concatenate([name_ids(g['name']) for g in gt_annos]) if rows else np.zeros(0, np.int32)


def pack_ground_truth(gt_annos):
    """``PackedGroundTruth`` of a ground-truth list, or the argument itself when it already is one.  It is a snapshot: pack
    again after changing an annotation.  An epoch loop packs its ground truth once and hands the result to
    ``kitti_eval_device`` in place of the list."""
    return gt_annos if isinstance(gt_annos, PackedGroundTruth) else PackedGroundTruth(gt_annos)


class Packed:
    """One packed input (the layout of include/sgv3d_hip.h) in ``buffer`` (uint8, pinned when asked for) and its counts."""
    __slots__ = ('buffer', 'M', 'TG', 'TD', 'pairs', 'tiles', 'ov_off', 'gt_num', 'dt_num')


def pack_annotations(gt_annos, dt_annos, pinned=False):
    gt = pack_ground_truth(gt_annos)
    M = len(dt_annos)
    assert M == len(gt.counts), 'one detection annotation per ground-truth annotation'
    dn = np.array([len(d['name']) for d in dt_annos], np.int64)
    if M and dn.max() > MAX_DETECTIONS:
        raise ValueError(f"an image has {int(dn.max())} detections; the device match handles at most {MAX_DETECTIONS}")
    drows = [np.concatenate([_f64(d['alpha'], 1), _f64(d['bbox'], 4), _f64(d['dimensions'], 3)[:, [1, 2, 0]], _f64(d['location'], 3),
                             _f64(d['rotation_y'], 1), _f64(d['score'], 1)], 1) for d in dt_annos]
    drows = np.concatenate(drows, 0) if drows else np.zeros((0, DT_FIELDS))
    if np.isnan(drows[:, 12]).any():
        raise ValueError("NaN detection scores cannot be ranked (the host path's sort is undefined for them too)")
    dcls = np.concatenate([name_ids(d['name'], dontcare=False) for d in dt_annos]) if M else np.zeros(0, np.int32)
    gn = gt.counts
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    p = Packed()
    p.M, p.TG, p.TD = M, int(gn.sum()), int(dn.sum())
    p.ov_off = off(gn * dn)
    tile_off = off(-(-dn // TILE) * -(-gn // TILE))
    p.pairs, p.tiles = int(p.ov_off[-1]), int(tile_off[-1])
    assert p.TG <= 2 ** 28 and p.TD < 2 ** 31 and p.tiles < 2 ** 31
    p.gt_num, p.dt_num = gn, dn
    sections = [(p.ov_off, np.int64), (off(gn), np.int32), (off(dn), np.int32), (tile_off, np.int32), (gt.rows, np.float64),
                (drows, np.float64), (gt.names, np.int32), (dcls, np.int32)]
    total = sum(_up8(np.asarray(a).size * np.dtype(t).itemsize) for a, t in sections)
    buf = torch.zeros(max(total, 8), dtype=torch.uint8)
    if pinned:
        buf = buf.pin_memory()
    view, o = buf.numpy(), 0
    for a, t in sections:
        n = np.asarray(a).size * np.dtype(t).itemsize
        view[o:o + n].view(t)[:] = np.asarray(a).reshape(-1)
        o += _up8(n)
    p.buffer = buf[:total] if total else buf[:0]
    return p


def _out_layout(ncell):
    """Offsets of precision, recall, orientation f64 [ncell, 41], num_thresholds i32 [ncell], status i32 -> (offsets, bytes)."""
    c = ncell * POINTS * 8
    return (0, c, 2 * c, 3 * c, 3 * c + ncell * 4), _up8(3 * c + ncell * 4 + 4)


def _split_outputs(raw, num_classes):
    ncell = 18 * num_classes
    o, _ = _out_layout(ncell)
    shape = (3, num_classes, 3, 2, POINTS)
    curve = lambda k: raw[o[k]:o[k] + ncell * POINTS * 8].view(np.float64).reshape(shape).copy()
    nthr = raw[o[3]:o[3] + ncell * 4].view(np.int32).reshape(shape[:-1]).copy()
    status = int(raw[o[4]:o[4] + 4].view(np.int32)[0])
    return curve(0), curve(1), curve(2), nthr, status


def _check_status(status):
    if status & 1:
        raise RuntimeError("kitti_eval_device: a cell produced more than 41 recall thresholds")
    if status & 2:
        raise RuntimeError("kitti_eval_device: the packed offsets do not agree with the totals, or an image has more than "
                           f"{MAX_DETECTIONS} detections")


def curves_host(packed, overlaps_bev, overlaps_3d, classes, min_overlaps, compute_aos, thresholds=None):
    """``sgv3d_kitti_eval_device_host`` over a ``Packed`` input -> (precision, recall, orientation [3, C, 3, 2, 41], num_thresholds
    [3, C, 3, 2], status).  ``overlaps_*``: float32 [pairs], image after image, each image's block [detections, ground truth].
    ``thresholds``: None, or a float64 array [3, C, 3, 2, 41] that receives every cell's recall thresholds."""
    lib = _lib.load()
    classes = np.ascontiguousarray(classes, np.int32)
    mo = np.ascontiguousarray(min_overlaps, np.float64)
    C = len(classes)
    assert mo.shape == (2, 3, C)
    bev = np.ascontiguousarray(overlaps_bev, np.float32).reshape(-1)
    d3 = np.ascontiguousarray(overlaps_3d, np.float32).reshape(-1)
    assert bev.size == packed.pairs and d3.size == packed.pairs
    assert thresholds is None or (thresholds.dtype == np.float64 and thresholds.flags.c_contiguous and thresholds.size == 18 * C * POINTS)
    _, nbytes = _out_layout(18 * C)
    raw = np.zeros(nbytes, np.uint8)
    o, _ = _out_layout(18 * C)
    base = raw.ctypes.data
    rc = lib.sgv3d_kitti_eval_device_host(packed.M, packed.TG, packed.TD, packed.pairs, packed.buffer.data_ptr(), packed.buffer.numel(),
                                          bev.ctypes.data if packed.pairs else None, d3.ctypes.data if packed.pairs else None, C,
                                          classes.ctypes.data, mo.ctypes.data, int(bool(compute_aos)), base + o[0], base + o[1],
                                          base + o[2], base + o[3], base + o[4],
                                          None if thresholds is None else thresholds.ctypes.data)
    _lib.check(rc, "sgv3d_kitti_eval_device_host")
    return _split_outputs(raw, C)


def curves_device(packed, classes, min_overlaps, compute_aos, device='cuda'):
    """The launches: one upload of ``packed.buffer``, ``sgv3d_kitti_eval_device``, one download.  Same return as ``curves_host``."""
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError("kitti_eval_device: the AP tables are computed on the GPU (there is no CPU path)")
    lib = _lib.load()
    classes = np.ascontiguousarray(classes, np.int32)
    mo = np.ascontiguousarray(min_overlaps, np.float64)
    C = len(classes)
    assert mo.shape == (2, 3, C)
    _, out_bytes = _out_layout(18 * C)
    o, _ = _out_layout(18 * C)
    in_bytes = _up8(packed.buffer.numel())
    ws = lib.sgv3d_kitti_eval_device_workspace_bytes(packed.M, packed.TG, packed.TD, packed.pairs, C)
    host_out = torch.empty(out_bytes, dtype=torch.uint8).pin_memory()
    with torch.cuda.device(dev):
        dbuf = torch.empty(in_bytes + out_bytes + max(ws, 8), dtype=torch.uint8, device=dev)
        if packed.buffer.numel():
            dbuf[:packed.buffer.numel()].copy_(packed.buffer, non_blocking=True)
        base = dbuf.data_ptr()
        out = base + in_bytes
        with hip_ops.prof("kitti_eval_device"):
            rc = lib.sgv3d_kitti_eval_device(packed.M, packed.TG, packed.TD, packed.pairs, packed.tiles, base, packed.buffer.numel(), C,
                                             classes.ctypes.data, mo.ctypes.data, int(bool(compute_aos)), out + out_bytes, ws,
                                             out + o[0], out + o[1], out + o[2], out + o[3], out + o[4], _lib.stream_handle(dev))
        _lib.check(rc, "sgv3d_kitti_eval_device")
        with hip_ops.prof("kitti_curves_to_host"):
            host_out.copy_(dbuf[in_bytes:in_bytes + out_bytes], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    return _split_outputs(host_out.numpy(), C)


def kitti_eval_device(gt_annos, dt_annos, current_classes, eval_types=('bbox', 'bev', '3d'), metric="R40", device='cuda'):
    """``kitti_eval`` with everything between the annotation arrays and the curves on the device.  ``gt_annos`` may be a
    ``PackedGroundTruth`` (``pack_ground_truth``)."""
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError("kitti_eval_device: the AP tables are computed on the GPU (there is no CPU path)")
    gt = pack_ground_truth(gt_annos)
    eval_types, classes, min_overlaps, compute_aos = eval_setup(gt.annos, dt_annos, current_classes, eval_types)
    if any(c not in (0, 1, 2, 3) for c in classes):
        raise ValueError("kitti_eval_device: classes are Car, Pedestrian, Cyclist and Bus (ids 0..3), as clean_data knows them")
    shape = (len(classes), 3, 2)
    if len(dt_annos) == 0:                                   # eval_class: all-zero curves for an empty set
        precision = orientation = np.zeros((3,) + shape + (POINTS,))
    else:
        packed = pack_annotations(gt, dt_annos, pinned=True)
        precision, _, orientation, _, status = curves_device(packed, classes, min_overlaps, 'aos' in eval_types, dev)
        _check_status(status)
    ap = get_mAP_R40 if metric == 'R40' else get_mAP
    pick = lambda kind, curves: ap(curves[_METRIC[kind]]) if kind in eval_types else None
    return eval_report(classes, min_overlaps, compute_aos, pick('bbox', precision), pick('bev', precision), pick('3d', precision),
                       ap(orientation[0]) if 'aos' in eval_types and 'bbox' in eval_types else None)
