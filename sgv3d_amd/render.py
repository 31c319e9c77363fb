"""Detections drawn on the device (csrc/render.hip): 3-D box wireframes on the camera frame, the boxes' footprints on a BEV
canvas and the SAM class mask laid over the frame.

Closes the annotate path: ``JpegDecoder`` -> model -> ``decode_device`` -> ``DetectionRenderer`` -> ``JpegEncoder``.  Frames
stay on the GPU as uint8 ``[B, H, W, 3]`` RGB; the detections are read where ``decode_device`` left them.  One upload (the
calibration blocks and label boxes), three launches whatever the batch, no download: ``status()`` is the only call that waits.

    r = DetectionRenderer(class_names, src_hw=(1080, 1920), bev=BevCanvas())
    out = r.draw_packed(frames, packed, img_metas, calib=[(Tr_velo_to_cam, K), ...])
    files = JpegEncoder(src_hw=(1080, 1920))(out.frames).files()

The geometry is the reference's (``get_lidar_3d_8points``, ``draw_box_3d``'s edges, ``pcl2xy_plane``, the ``int()``
truncations) in float64; the pixels of a line follow this project's own integer rule (DESIGN.md "Rendering detections"), not
OpenCV's.  There is no CPU fallback: host tensors, wrong dtypes or shapes raise before any launch."""
import csv
import ctypes
import io
import math
import os

import numpy as np
import torch

from . import _lib, hip_ops
from .evaluators.device_kitti import _CALIB, calib_block, class_table
from .evaluators.result2kitti import category_map_dair

__all__ = ['DetectionRenderer', 'BevCanvas', 'RenderOutput', 'RenderError', 'label_boxes', 'default_class_colors', 'EOVERFLOW',
           'MAX_SIDE', 'MAX_BOXES', 'MASK_PALETTE']

EOVERFLOW = 1            # include/sgv3d_hip.h SGV3D_RENDER_EOVERFLOW
MAX_SIDE = 8192          # SGV3D_RENDER_MAX_SIDE
MAX_BOXES = 1024         # SGV3D_RENDER_MAX_BOXES

# visual_utils.color_map, its BGR tuples turned to RGB; any other class is white
_NAME_COLORS = {'car': (0, 255, 0), 'bus': (255, 255, 0), 'van': (255, 255, 0), 'truck': (255, 255, 0),
                'pedestrian': (0, 255, 255), 'cyclist': (255, 0, 0)}
# RGB per mask class id 0..6 (mask_image() writes id * 40; id 0 is background and never blended)
MASK_PALETTE = ((0, 0, 0), (0, 255, 0), (255, 255, 0), (0, 255, 255), (255, 0, 0), (255, 0, 255), (0, 128, 255))


class RenderError(ValueError):
    """Arguments the renderer does not take."""


def default_class_colors(class_names):
    """uint8 [num_classes, 3]: the reference's colour per class name, white for a name it does not list."""
    return np.array([_NAME_COLORS.get(n, (255, 255, 255)) for n in class_names], np.uint8).reshape(-1, 3)


class BevCanvas:
    """``pcd_vis``'s canvas: ``PointCloudFilter(side_range, fwd_range, res)``'s mesh grid and the two integer offsets of
    ``pcl2xy_plane``, computed here in Python as the reference computes them."""

    def __init__(self, side_range=(-60, 60), fwd_range=(0, 100), res=0.1):
        self.side_range, self.fwd_range, self.res = tuple(side_range), tuple(fwd_range), float(res)
        if not (self.res > 0 and math.isfinite(self.res)):
            raise RenderError(f"BevCanvas: res {res!r} is not a positive number")
        self.width = 1 + int((self.side_range[1] - self.side_range[0]) / self.res)
        self.height = 1 + int((self.fwd_range[1] - self.fwd_range[0]) / self.res)
        self.x_off = int(np.floor(self.side_range[0] / self.res))
        self.y_off = int(np.ceil(self.fwd_range[1] / self.res))
        if not (1 <= self.width <= MAX_SIDE and 1 <= self.height <= MAX_SIDE):
            raise RenderError(f"BevCanvas: {self.height} x {self.width} pixels, sides must lie in [1, {MAX_SIDE}]")
        if max(abs(self.x_off), abs(self.y_off)) >= 2 ** 31:
            raise RenderError("BevCanvas: the pixel offsets do not fit 32 bits")


def _fold(angle):
    """One turn back towards zero for an angle beyond a full turn either way; anything inside (-2 pi, 2 pi) stays."""
    if angle > 2 * np.pi:
        return angle - 2 * np.pi
    if angle < -2 * np.pi:
        return angle + 2 * np.pi
    return angle


def label_boxes(label_txt, Tr_cam2lidar):
    """A KITTI label file (its path or its text) -> float64 ``[m, 7]`` rows ``(x, y, z_bottom, ex, ey, h, yaw)`` in the lidar frame,
    the boxes the reference's ``read_label_bboxes`` (evaluators/result2kitti.py) hands to ``get_lidar_3d_8points``: ``box_corner``
    of a row gives that function's corners.  The rule, per line of 15 space-separated columns
    (type, truncated, occluded, alpha, four bbox columns, h, w, l, x, y, z in the camera frame, rotation_y):

    * a line whose three dimensions sum to 0 gives no row;
    * ``rotation_y`` is taken as written, except where ``alpha > pi``: there it is rebuilt as ``(alpha - 2 pi) + arctan2(x, z)``
      with the arctan2 evaluated on float32 ``x`` and ``z``, brought back by a turn if it leaves ``[-pi, pi]``;
    * the angle is folded by ``_fold`` and ``yaw = pi / 2 - rotation_y``;
    * the camera-frame location goes through ``Tr_cam2lidar`` (4 x 4); KITTI's location is the bottom centre, which the
      reference lifts by ``h / 2`` and steps back down again, both roundings kept; the extents are ``(l, w, h)``."""
    text = str(label_txt)
    if '\n' not in text and os.path.exists(text):
        with open(text, 'r') as fp:
            text = fp.read()
    cam2lidar = np.asarray(Tr_cam2lidar)
    rows = []
    # csv, not str.split: a quoted or empty column parses as it does for the reference's reader
    for cols in csv.reader(io.StringIO(text), delimiter=' '):
        if not cols:
            continue
        alpha = float(cols[3])
        h, w, l = (float(v) for v in cols[8:11])
        x, y, z = (float(v) for v in cols[11:14])
        rot_y = float(cols[14])
        if alpha > np.pi:
            rot_y = (alpha - 2 * np.pi) + np.arctan2(np.float32(x), np.float32(z))
            if rot_y > np.pi:
                rot_y -= 2 * np.pi
            if rot_y < -np.pi:
                rot_y += 2 * np.pi
        if l + w + h == 0:
            continue
        yaw = 0.5 * np.pi - _fold(rot_y)
        centre = np.matmul(cam2lidar, np.array([[x], [y], [z], [1.0]]))[:3, 0]
        z_bottom = float(centre[2] + 0.5 * h) - h / 2
        rows.append([float(centre[0]), float(centre[1]), z_bottom, l, w, h, float(yaw)])
    return np.array(rows, np.float64).reshape(-1, 7)


class RenderOutput:
    """``frames`` uint8 [B, H, W, 3] and ``bev`` uint8 [B, Hb, Wb, 3] (or None) on the GPU; ``status()`` waits."""

    def __init__(self, frames, bev, status):
        self.frames, self.bev, self._status = frames, bev, status

    def status(self):
        """int32 [B] on the host: 0, or ``EOVERFLOW`` for a sample that was copied through unannotated.  Waits for the device."""
        return self._status.cpu().numpy()


class DetectionRenderer:
    def __init__(self, class_names, src_hw=(1080, 1920), max_boxes=256, thickness=2, z_near=0.5, bev=None, score_threshold=0.45,
                 category_map=category_map_dair, palette=None, mask_alpha=96, class_colors=None, label_color=(255, 0, 0),
                 bev_pred_color=(0, 0, 255), bev_label_color=(255, 0, 0)):
        self.class_names = list(class_names)
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        if not (1 <= len(self.class_names) <= 64):
            raise RenderError(f"DetectionRenderer: {len(self.class_names)} classes, 1..64 are supported")
        if not all(1 <= s <= MAX_SIDE for s in self.src_hw):
            raise RenderError(f"DetectionRenderer: src_hw {self.src_hw}, sides must lie in [1, {MAX_SIDE}]")
        if not (1 <= int(max_boxes) <= MAX_BOXES):
            raise RenderError(f"DetectionRenderer: max_boxes {max_boxes} outside [1, {MAX_BOXES}]")
        if not (1 <= int(thickness) <= 15):
            raise RenderError(f"DetectionRenderer: thickness {thickness} outside [1, 15]")
        if not (float(z_near) > 0 and math.isfinite(float(z_near))):
            raise RenderError(f"DetectionRenderer: z_near {z_near!r} is not a positive number")
        if not (0 <= int(mask_alpha) <= 256):
            raise RenderError(f"DetectionRenderer: mask_alpha {mask_alpha} outside [0, 256]")
        if bev is not None and not isinstance(bev, BevCanvas):
            raise RenderError("DetectionRenderer: bev is a BevCanvas or None")
        self.bev = bev
        colors = default_class_colors(self.class_names) if class_colors is None else np.asarray(class_colors)
        if colors.shape != (len(self.class_names), 3):
            raise RenderError(f"DetectionRenderer: class_colors has shape {colors.shape}, not {(len(self.class_names), 3)}")
        pal = np.asarray(MASK_PALETTE if palette is None else palette)
        if pal.shape != (7, 3):
            raise RenderError(f"DetectionRenderer: palette has shape {pal.shape}, not (7, 3): one RGB row per mask class id 0..6")
        d = _lib.RenderDesc()
        d.height, d.width = self.src_hw
        d.max_boxes, d.thickness, d.num_classes, d.mask_alpha = int(max_boxes), int(thickness), len(self.class_names), int(mask_alpha)
        d.score_thr, d.z_near = float(score_threshold), float(z_near)
        if bev is not None:
            d.bev_h, d.bev_w, d.bev_x_off, d.bev_y_off, d.bev_res = bev.height, bev.width, bev.x_off, bev.y_off, bev.res
        table = class_table(self.class_names, category_map)
        for k in range(64):
            d.class_table[k] = int(table[k]) if k < len(table) else -1
        for name, src, n in (("class_colors", colors, 3 * len(self.class_names)), ("label_color", label_color, 3),
                             ("bev_pred_color", bev_pred_color, 3), ("bev_label_color", bev_label_color, 3), ("palette", pal, 21)):
            flat = np.asarray(src).reshape(-1)
            if flat.size != n or flat.min() < 0 or flat.max() > 255:
                raise RenderError(f"DetectionRenderer: {name} is not {n // 3} RGB rows of 0..255")
            arr = getattr(d, name)
            for k in range(n):
                arr[k] = int(flat[k])
        self._desc = d

    # ------------------------------------------------------------------------------------------------ input side
    def _desc_for(self, B, N, m, f64):
        d = _lib.RenderDesc.from_buffer_copy(self._desc)
        d.batch, d.n, d.m, d.f64_inputs = B, N, m, int(f64)
        return d

    def _check_images(self, who, frames, masks, out, B):
        H, W = self.src_hw
        for name, t, shape in (("frames", frames, (B, H, W, 3)), ("masks", masks, (B, H, W)), ("out", out, (B, H, W, 3))):
            if t is None and name != "frames":
                continue
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RenderError(f"{who}: {name} must be a tensor on the GPU (there is no CPU path)")
            if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
                raise RenderError(f"{who}: {name} is {t.dtype} {tuple(t.shape)}, a contiguous uint8 {shape} is needed")
            if t.device != frames.device:
                raise RenderError(f"{who}: {name} is on {t.device}, frames on {frames.device}")

    def _blocks(self, img_metas, calib):
        if calib is None:
            raise RenderError("DetectionRenderer: calib=[(Tr_velo_to_cam, K), ...] or a float64 [B, 33] array of calib_block rows")
        if isinstance(calib, np.ndarray) and calib.shape == (len(img_metas), _CALIB):
            return calib.astype(np.float64)
        if len(calib) != len(img_metas):
            raise RenderError(f"DetectionRenderer: {len(calib)} calibrations for {len(img_metas)} samples")
        return np.stack([calib_block(Tr, K, meta.get('ego2global_rotation', (1.0, 0.0, 0.0, 0.0)),
                                     meta.get('ego2global_translation', (0.0, 0.0, 0.0)))
                         for (Tr, K), meta in zip(calib, img_metas)])

    def _run(self, who, dev, B, N, boxes_ptr, scores_ptr, f64, labels_ptr, counts_ptr, counts_host, frames, img_metas, calib, labels,
             masks, out, hold):
        """One upload and three launches on the current stream of ``dev``.  ``counts_ptr`` None: the counts come from the host
        (``counts_host``) and ride in the upload.  ``hold``: tensors the launches read."""
        self._check_images(who, frames, masks, out, B)
        blocks = self._blocks(img_metas, calib)
        m, lab = 0, None
        if labels is not None:
            if len(labels) != B:
                raise RenderError(f"{who}: {len(labels)} label lists for {B} samples")
            lab = [np.asarray(v, np.float64).reshape(-1, 7) for v in labels]
            m = max(1, max(len(v) for v in lab))
        # the upload: calib f64 [B, 33] | label boxes f64 [B, m, 7] | label counts i32 [B] | counts i32 [B]
        lab_off, lc_off = B * _CALIB * 8, B * _CALIB * 8 + B * m * 56
        cnt_off = lc_off + B * 4
        stage = np.zeros(cnt_off + B * 4, np.uint8)
        stage[:lab_off].view(np.float64)[:] = blocks.reshape(-1)
        if lab is not None:
            lb = stage[lab_off:lc_off].view(np.float64).reshape(B, m, 7)
            for b, v in enumerate(lab):
                lb[b, :len(v)] = v
            stage[lc_off:cnt_off].view(np.int32)[:] = [len(v) for v in lab]
        if counts_host is not None:
            stage[cnt_off:].view(np.int32)[:] = counts_host
        desc = self._desc_for(B, N, m, f64)
        lib = _lib.load()
        nws = lib.sgv3d_render_workspace_bytes(ctypes.byref(desc))
        if nws == 0:
            _lib.check(-1, "sgv3d_render_workspace_bytes")
        with torch.cuda.device(dev):
            dstage = torch.empty(stage.size, dtype=torch.uint8, device=dev)
            dstage.copy_(torch.from_numpy(stage).pin_memory(), non_blocking=True)
            work = torch.empty(nws, dtype=torch.uint8, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            if out is None:
                out = torch.empty_like(frames)
            bev = None
            if self.bev is not None:
                bev = torch.empty(B, self.bev.height, self.bev.width, 3, dtype=torch.uint8, device=dev)
            base = dstage.data_ptr()
            with hip_ops.prof("render_detections"):
                rc = lib.sgv3d_render_detections(
                    ctypes.byref(desc), boxes_ptr, scores_ptr, labels_ptr, counts_ptr if counts_ptr is not None else base + cnt_off,
                    base, base + lab_off if lab is not None else None, base + lc_off if lab is not None else None,
                    frames.data_ptr(), _lib.ptr(masks), out.data_ptr(), _lib.ptr(bev), status.data_ptr(), work.data_ptr(), nws,
                    _lib.stream_handle(dev))
            _lib.check(rc, "sgv3d_render_detections")
        del hold, dstage, work              # the caching allocator keeps them alive for work already enqueued on this stream
        return RenderOutput(out, bev, status)

    def draw_packed(self, frames, packed, img_metas, calib=None, labels=None, masks=None, out=None):
        """``packed``: ``decode_device``'s buffer for ``len(img_metas)`` samples, read in place on its device.  ``labels``: per
        sample a ``[m, 7]`` array of ``label_boxes`` rows.  ``out=frames`` draws in place."""
        B = len(img_metas)
        if B < 1 or not torch.is_tensor(packed) or packed.dtype != torch.uint8 or not packed.is_contiguous():
            raise RenderError("DetectionRenderer.draw_packed: packed must be decode_device's contiguous uint8 buffer")
        N = (packed.numel() - 4 * B) // (44 * B)
        if N < 1 or packed.numel() != B * N * 44 + 4 * B:
            raise RenderError("DetectionRenderer.draw_packed: not a decode_device buffer for this batch size")
        if not packed.is_cuda:
            raise RenderError("DetectionRenderer.draw_packed: the packed detections must be on the GPU (there is no CPU path)")
        if torch.is_tensor(frames) and frames.is_cuda and frames.device != packed.device:
            raise RenderError(f"DetectionRenderer.draw_packed: packed is on {packed.device}, frames on {frames.device}")
        p = packed.data_ptr()
        return self._run("DetectionRenderer.draw_packed", packed.device, B, N, p, p + B * N * 36, False, p + B * N * 40,
                         p + B * N * 44, None, frames, img_metas, calib, labels, masks, out, packed)

    def draw(self, frames, results, img_metas, calib=None, labels=None, masks=None, out=None):
        """``results``: ``[[boxes, scores, labels], ...]`` as ``get_bboxes`` returns them, like ``KittiDetections.add``.  Host
        tensors are uploaded; the drawing itself always runs on the device."""
        B = len(img_metas)
        if B < 1 or len(results) != B:
            raise RenderError(f"DetectionRenderer.draw: {len(results)} results for {B} samples")
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise RenderError("DetectionRenderer.draw: frames must be a tensor on the GPU (there is no CPU path)")
        dev = frames.device
        rows = []
        for boxes, scores, labs in results:
            boxes = boxes.tensor if hasattr(boxes, 'tensor') else boxes
            boxes, scores, labs = (torch.as_tensor(v) for v in (boxes, scores, labs))
            rows.append((boxes.reshape(-1, 9), scores.reshape(-1), labs.reshape(-1)))
        counts = np.array([int(r[0].shape[0]) for r in rows], np.int32)
        N = max(1, int(counts.max()))
        f64 = any(r[0].dtype == torch.float64 for r in rows)
        dt = torch.float64 if f64 else torch.float32
        with torch.cuda.device(dev):
            tb = torch.zeros(B, N, 9, dtype=dt, device=dev)
            ts = torch.zeros(B, N, dtype=dt, device=dev)
            tl = torch.zeros(B, N, dtype=torch.int32, device=dev)
            for b, (boxes, scores, labs) in enumerate(rows):
                n = int(counts[b])
                if n:
                    tb[b, :n].copy_(boxes.to(dev, non_blocking=True))
                    ts[b, :n].copy_(scores.to(dev, non_blocking=True))
                    tl[b, :n].copy_(labs.to(dev, non_blocking=True))
        return self._run("DetectionRenderer.draw", dev, B, N, tb.data_ptr(), ts.data_ptr(), f64, tl.data_ptr(), None, counts, frames,
                         img_metas, calib, labels, masks, out, (tb, ts, tl))
