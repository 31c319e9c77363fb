"""Detections -> KITTI annotations on the device (csrc/result2kitti.hip), without the results JSON, the label files
and their parser.

``RoadSideEvaluator.evaluate`` turns every detection into a dict, a JSON record, about twenty small numpy calls, a line
of text and back into arrays (``_format_bbox`` -> ``result2kitti`` -> ``kitti_common.get_label_annos``).
``KittiDetections`` collects the same annotations from the detections where they already are: one kernel launch per
batch reads ``decode_device``'s packed buffer in place, applies the score test and the category map first, and writes
the kept rows, rounded as the label files round them, into a buffer that one asynchronous copy brings to pinned host
memory.  ``annos()`` is what ``get_label_annos`` returns for the file chain's files, bit for bit; ``write()`` writes those
files (SGV3D's semi-supervised stage reads them as pseudo labels).  The file chain stays as the yardstick.

Nothing here waits for the device before ``annos()`` / ``write()``: calibrations are read on the host (cached per token),
uploaded in one copy per call, and finished copies are collected with a non-blocking event query."""
import ctypes
import json
import os

import numpy as np
import torch

from .. import _lib, hip_ops
from .det_evaluators import _quat_matrix
from .result2kitti import (_numeric_id, category_map_dair, load_calib_dair, load_calib_dair_json, load_calib_rope3d)

__all__ = ['KittiDetections', 'KITTI_NAMES', 'FIELDS']

KITTI_NAMES = ('Car', 'Pedestrian', 'Cyclist')          # the kernel's class ids 0, 1, 2
FIELDS = 13                                             # alpha, x1, y1, x2, y2, h, l, w, x, y, z, rotation_y, score
_CALIB = 33                                             # Tr_velo_to_cam 3x4 | camera matrix 3x3 | ego2global 3x3 | translation 3


def _up8(n):
    return (n + 7) // 8 * 8


def calib_block(Tr, K, rotation=(1.0, 0.0, 0.0, 0.0), translation=(0.0, 0.0, 0.0)):
    """The 33 doubles the kernel reads for one frame: what ``_convert`` takes from (Tr, K) and ``_format_bbox`` from the
    frame's ego2global quaternion (w, x, y, z) and translation."""
    out = np.empty(_CALIB, np.float64)
    out[:12] = np.asarray(Tr, np.float64)[:3, :4].reshape(-1)
    out[12:21] = np.asarray(K, np.float64)[:3, :3].reshape(-1)
    out[21:30] = _quat_matrix(np.array(rotation, np.float64)).reshape(-1)
    out[30:33] = np.array(translation, np.float64)
    return out


def class_table(class_names, category_map):
    """int8 [num_classes]: the detector's class index -> 0 Car, 1 Pedestrian, 2 Cyclist, -1 not in the category map."""
    return np.array([KITTI_NAMES.index(category_map[n]) if n in category_map else -1 for n in class_names], np.int8)


class KittiDetections:
    def __init__(self, class_names, data_root=None, category_map=category_map_dair, score_threshold=0.45,
                 img_size=(1920, 1080), max_det=256, token_map=None):
        self.class_names = list(class_names)
        self.table = class_table(self.class_names, category_map)
        self.data_root = data_root
        self.score_threshold = float(score_threshold)
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.max_det = int(max_det)
        assert self.max_det >= 1 and 1 <= len(self.class_names) <= 64
        self.sample_id_of = _numeric_id
        # the loader RoadSideEvaluator.evaluate would pick for this root
        if data_root is None:
            self.load_calib = None
        elif 'dair-v2x-i-kitti' in data_root or 'rope3d-kitti' in data_root:
            self.load_calib = lambda tok: load_calib_dair(
                os.path.join(data_root, "training/calib", "{:06d}".format(_numeric_id(tok)) + ".txt"))
        elif 'dair-v2x-i' in data_root:
            self.load_calib = lambda tok: load_calib_dair_json(data_root, _numeric_id(tok))
        else:
            self.load_calib = lambda tok: load_calib_rope3d(data_root, tok)
            if token_map is None:
                token_map = "data/rope3d-kitti/map_token2id.json"       # the path result2kitti_rope3d opens
        if token_map is not None:
            if not isinstance(token_map, dict):
                with open(token_map) as fp:
                    token_map = json.load(fp)
            self.sample_id_of = lambda tok: int(token_map[tok])
        self._calib = {}            # token -> the 21 doubles of (Tr, K)
        self._pending = []          # (event, pinned buffer, stage bytes, tokens) of calls whose copy may still be in flight
        self._free = {}             # pinned buffers ready for reuse, by size
        self._frames = []           # (token, kept, cls i32 [m], fields f64 [m, 13]) in arrival order

    # ------------------------------------------------------------------------------------------------ input side
    def _blocks(self, img_metas, calib):
        out = np.empty((len(img_metas), _CALIB), np.float64)
        for i, meta in enumerate(img_metas):
            tok = meta['token']
            if calib is not None:
                out[i, :21] = calib_block(*calib[i])[:21]
            else:
                if tok not in self._calib:
                    if self.load_calib is None:
                        raise ValueError("KittiDetections without a data_root needs calib=[(Tr, K), ...]")
                    self._calib[tok] = calib_block(*self.load_calib(tok))[:21]
                out[i, :21] = self._calib[tok]
            out[i, 21:30] = _quat_matrix(np.array(meta.get('ego2global_rotation', (1.0, 0.0, 0.0, 0.0)), np.float64)).reshape(-1)
            out[i, 30:33] = np.array(meta.get('ego2global_translation', (0.0, 0.0, 0.0)), np.float64)
        return out

    def _pinned(self, nbytes):
        pool = self._free.get(nbytes)
        return pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def _run(self, dev, B, N, boxes_ptr, scores_ptr, f64, labels_ptr, counts_ptr, counts_host, img_metas, calib, hold):
        """One upload, one launch, one download, all enqueued on the current stream of ``dev``.  ``counts_ptr`` None: the
        counts come from the host (``counts_host``) and ride in the upload.  ``hold``: tensors the launch reads."""
        self._collect(block=False)
        lib, M = _lib.load(), self.max_det
        stage_bytes = B * _CALIB * 8 + _up8(B * 4)
        cls_off = B * 4
        fields_off = _up8(cls_off + B * M * 4)
        out_bytes = fields_off + B * M * FIELDS * 8
        host = self._pinned(stage_bytes + out_bytes)
        stage = host[:stage_bytes].numpy()
        stage[:B * _CALIB * 8].view(np.float64)[:] = self._blocks(img_metas, calib).reshape(-1)
        stage[B * _CALIB * 8:B * _CALIB * 8 + B * 4].view(np.int32)[:] = counts_host if counts_host is not None else 0
        nws = lib.sgv3d_detections_to_kitti_workspace_bytes(B, N)
        with torch.cuda.device(dev):
            dbuf = torch.empty(stage_bytes + out_bytes + nws, dtype=torch.uint8, device=dev)
            dbuf[:stage_bytes].copy_(host[:stage_bytes], non_blocking=True)
            base = dbuf.data_ptr()
            out = base + stage_bytes
            with hip_ops.prof("detections_to_kitti"):
                rc = lib.sgv3d_detections_to_kitti(
                    B, N, boxes_ptr, scores_ptr, int(f64), labels_ptr,
                    counts_ptr if counts_ptr is not None else base + B * _CALIB * 8, base,
                    self.table.ctypes.data_as(ctypes.c_void_p), len(self.table), self.score_threshold, self.img_size[0],
                    self.img_size[1], M, 4, out + out_bytes, nws, out + fields_off, out + cls_off, out, _lib.stream_handle(dev))
            _lib.check(rc, "sgv3d_detections_to_kitti")
            with hip_ops.prof("kitti_annos_to_host"):
                host[stage_bytes:].copy_(dbuf[stage_bytes:stage_bytes + out_bytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        del hold, dbuf                      # the caching allocator keeps both alive for work already enqueued on this stream
        self._pending.append((ev, host, stage_bytes, [m['token'] for m in img_metas]))

    def add_packed(self, packed, img_metas, calib=None):
        """``packed``: ``decode_device``'s buffer for ``len(img_metas)`` samples, read in place on its device."""
        B = len(img_metas)
        assert B >= 1 and torch.is_tensor(packed) and packed.dtype == torch.uint8 and packed.is_contiguous()
        if not packed.is_cuda:
            raise RuntimeError("KittiDetections.add_packed: the packed detections must be on the GPU (there is no CPU path)")
        N = (packed.numel() - 4 * B) // (44 * B)
        assert N >= 1 and packed.numel() == B * N * 44 + 4 * B, "not a decode_device buffer for this batch size"
        p = packed.data_ptr()
        self._run(packed.device, B, N, p, p + B * N * 36, False, p + B * N * 40, p + B * N * 44, None, img_metas, calib, packed)

    def add(self, results, img_metas, calib=None):
        """``results``: ``[[boxes, scores, labels], ...]`` as ``get_bboxes`` returns them (box objects with ``.tensor``
        included).  Host tensors are uploaded; the conversion itself always runs on the device."""
        B = len(img_metas)
        assert B >= 1 and len(results) == B
        if not torch.cuda.is_available():
            raise RuntimeError("KittiDetections.add: no GPU (there is no CPU path)")
        rows, dev = [], None
        for boxes, scores, labels in results:
            boxes = boxes.tensor if hasattr(boxes, 'tensor') else boxes
            boxes, scores, labels = (torch.as_tensor(v) for v in (boxes, scores, labels))
            if dev is None and boxes.is_cuda:
                dev = boxes.device
            rows.append((boxes.reshape(-1, 9), scores.reshape(-1), labels.reshape(-1)))
        dev = dev if dev is not None else torch.device('cuda', torch.cuda.current_device())
        counts = np.array([int(r[0].shape[0]) for r in rows], np.int32)
        N = max(1, int(counts.max()))
        # float64 boxes (what the file chain's JSON carries) are read as they are; anything else as float32, like the decode's
        f64 = any(r[0].dtype == torch.float64 for r in rows)
        dt = torch.float64 if f64 else torch.float32
        with torch.cuda.device(dev):
            tb = torch.zeros(B, N, 9, dtype=dt, device=dev)
            ts = torch.zeros(B, N, dtype=dt, device=dev)
            tl = torch.zeros(B, N, dtype=torch.int32, device=dev)
            for b, (boxes, scores, labels) in enumerate(rows):
                n = int(counts[b])
                if n:
                    tb[b, :n].copy_(boxes.to(dev, non_blocking=True))
                    ts[b, :n].copy_(scores.to(dev, non_blocking=True))
                    tl[b, :n].copy_(labels.to(dev, non_blocking=True))
        self._run(dev, B, N, tb.data_ptr(), ts.data_ptr(), f64, tl.data_ptr(), None, counts, img_metas, calib, (tb, ts, tl))

    # ------------------------------------------------------------------------------------------------ output side
    def _collect(self, block):
        """Move finished calls from pinned memory into per-frame arrays; ``block=False`` never waits for the device."""
        M = self.max_det
        while self._pending:
            ev, host, stage_bytes, tokens = self._pending[0]
            if not ev.query():
                if not block:
                    return
                ev.synchronize()
            self._pending.pop(0)
            B = len(tokens)
            out = host[stage_bytes:].numpy()
            fields_off = _up8(B * 4 + B * M * 4)
            kept = out[:B * 4].view(np.int32)
            cls = out[B * 4:B * 4 + B * M * 4].view(np.int32).reshape(B, M)
            fields = out[fields_off:].view(np.float64).reshape(B, M, FIELDS)
            for b, tok in enumerate(tokens):
                m = min(int(kept[b]), M)
                self._frames.append((tok, int(kept[b]), cls[b, :m].copy(), fields[b, :m].copy()))
            self._free.setdefault(host.numel(), []).append(host)

    def _by_sample(self):
        self._collect(block=True)
        by_token = {}
        for tok, kept, cls, fields in self._frames:
            if kept > self.max_det:
                raise RuntimeError(f"frame {tok!r}: {kept} detections pass the score test and the category map, "
                                   f"max_det is {self.max_det}")
            by_token.setdefault(tok, []).append((cls, fields))
        by_id = {}
        for tok, parts in by_token.items():              # (two tokens with one sample id: the later one wins, as its file would)
            by_id[self.sample_id_of(tok)] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        return by_id

    def annos(self):
        """-> ``(dt_annos, image_ids)``: what ``kitti_common.get_label_annos(folder, return_ids=True)`` returns for the label
        files of these detections.  Waits for the device once."""
        by_id = self._by_sample()
        ids = sorted(by_id)
        annos = []
        for idx in ids:
            cls, f = by_id[idx]
            n = len(cls)
            annos.append({
                'name': np.array([KITTI_NAMES[c] for c in cls]),
                'truncated': np.zeros(n), 'occluded': np.zeros(n),
                'alpha': f[:, 0].copy(), 'bbox': f[:, 1:5].copy(),
                'dimensions': f[:, [7, 5, 6]].copy(),             # written h, l, w; read back as get_label_anno reorders them
                'location': f[:, 8:11].copy(), 'rotation_y': f[:, 11].copy(), 'score': f[:, 12].copy(),
                'index': np.arange(n, dtype=np.int32), 'group_ids': np.arange(n, dtype=np.int32),
                'image_idx': np.array([idx] * n, dtype=np.int64)})
        return annos, ids

    def write(self, results_path):
        """Write ``results_path/data/%06d.txt`` as ``result2kitti`` does; returns that folder."""
        folder = os.path.join(results_path, "data")
        os.makedirs(folder, exist_ok=True)
        for idx, (cls, f) in self._by_sample().items():
            with open(os.path.join(folder, "{:06d}".format(idx) + ".txt"), "w") as fp:
                for c, row in zip(cls, f.tolist()):
                    fp.write(" ".join([KITTI_NAMES[c], "0", "0"] + [repr(v) for v in row]) + "\n")
        return folder
