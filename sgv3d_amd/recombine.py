"""Frame recombination on the device (csrc/recombine.hip): SGV3D's semi-supervised data generation.

The reference's ``scripts/data_preprocess/recombine_strategy.py`` builds every frame of ``train_ssdg`` on the host in
numpy float64: three labeled or pseudo-labeled frames are warped into the camera of a background frame, matched to its
brightness, their objects gated by 2-D IoU, pasted with their class mask, and the labels rewritten in the destination
camera.  ``FrameRecombiner`` does the same on frames that are already on the GPU (``JpegDecoder``'s output shape) in
four launches per batch; its frames and masks go straight into ``TrainAugmenter`` / ``ImagePreprocessor.mask`` (online
copy-paste augmentation) or through ``write`` into the generated split (offline).

The class-id masks (values 0..6) come from the caller.  ``sgv3d_amd.sam_masks.get_sam_mask`` / ``mask_images`` draw them with SAM
on the device as the reference does; the stand-in of DESIGN.md section 17 remains available: each frame's
stored mask (``mask_image // 40``, what the reference's first stage writes) in place of the masks SAM would draw inside the
accepted boxes.  SAM's weights are still not available to this project, so nothing here has run with them.

There is no CPU path: ``combine`` needs the GPU.  ``load_sample``, ``sample_order`` and ``write`` are host file handling.
"""
import csv
import ctypes
import math
import os

import numpy as np

from . import _lib

__all__ = ['FrameRecombiner', 'RecombineResult', 'NAMES', 'FOCUS', 'sample_order', 'draw_order', 'load_sample', 'get_denorm', 'homography',
           'frame_descriptors', 'pack_objects', 'label_lines', 'write', 'FRAME_DTYPE']

FOCUS = ("car", "van", "truck", "bus", "pedestrian", "cyclist")              # cls_focus: the kernel's classes 0..5
NAMES = FOCUS + ("bicycle", "tricyclist", "motorcycle", "motorcyclist")      # color_map's keys: the names load_annos keeps
MAX_SOURCES = 3
OBJ_COLS, ROW_COLS = 30, 15

# mirror of sgv3d_recombine_frame (include/sgv3d_hip.h)
FRAME_DTYPE = np.dtype([('dest', 'i4'), ('n_src', 'i4'), ('src', 'i4', 3), ('obj0', 'i4'), ('n_obj', 'i4', 4),
                        ('minv', 'f8', (3, 9)), ('delta', 'f8', (3, 3)), ('tr', 'f8', 12), ('p2', 'f8', 12)])
assert FRAME_DTYPE.itemsize == 520


def _up(n, a=256):
    return (n + a - 1) // a * a


# ------------------------------------------------------------------------------------------------------------- host side
def sample_order(n, rnd, ratio=1.0):
    """The reference's draw over a source's ``n`` selected objects: ``random.sample(objects, int(ratio * n))`` as indices."""
    return rnd.sample(range(n), int(ratio * n))


def draw_order(objects, rnd, in_view=None, ratio=1.0):
    """The walk order of one source's objects as ``objects_combine_tools`` draws it: ``random.sample`` over the ``cls_focus``
    objects that ``update_bbox_info`` kept (``in_view``; all of them if not given), which consumes the generator as the
    reference does; the other objects follow in their stored order (the gate drops them wherever they stand)."""
    n = len(objects['names'])
    ok = np.ones(n, bool) if in_view is None else np.asarray(in_view, bool)
    selected = [i for i in range(n) if objects['names'][i].lower() in FOCUS and ok[i]]
    drawn = [selected[k] for k in sample_order(len(selected), rnd, ratio)]
    return drawn + [i for i in range(n) if i not in selected]


def _in_view(corners, delta, Tr, P2):
    """``update_bbox_info``'s test per object: not (xmax <= 0 or ymax <= 0) of the corners projected into the destination."""
    c = np.asarray(corners, np.float64).reshape(-1, 3, 8) + np.asarray(delta, np.float64)[None, :, None]
    cam = np.einsum('rk,nkc->nrc', Tr[:3, :3], c) + Tr[:3, 3][None, :, None]
    h = np.einsum('rk,nkc->nrc', P2[:3, :3], cam) + P2[:3, 3][None, :, None]
    with np.errstate(all='ignore'):
        u, v = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
    return ~((u.max(axis=1) <= 0) | (v.max(axis=1) <= 0)) if len(c) else np.zeros(0, bool)


def homography(Tr_src, P2_src, Tr_dest, P2_dest):
    """``get_M`` on the 3x3 blocks -> (M, inv(M)) with M = K_d R_d R_s^-1 K_s^-1.  The products are float64; a float32 P2
    (what ``load_sample`` and the reference's calib loader return) is inverted by numpy in float32 first, as the reference
    inverts it, so the generated pixels are the reference's."""
    R, K = np.asarray(Tr_src)[:3, :3], np.asarray(P2_src)[:3, :3]          # the arrays' own dtypes: see the docstring
    R_r, K_r = np.asarray(Tr_dest)[:3, :3], np.asarray(P2_dest)[:3, :3]
    M = np.matmul(np.matmul(np.matmul(K_r, R_r), np.linalg.inv(R)), np.linalg.inv(K))
    return M, np.linalg.inv(M)


def get_denorm(Tr_ego2cam):
    """The ground plane (a, b, c, d) in the camera frame from three ground points of the ego frame."""
    pts = np.array([[0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 1.0], [1.0, 1.0, 0.0, 1.0]])
    p = np.matmul(np.asarray(Tr_ego2cam, np.float64), pts.T).T
    a1, b1, c1 = p[1, 0] - p[0, 0], p[1, 1] - p[0, 1], p[1, 2] - p[0, 2]
    a2, b2, c2 = p[2, 0] - p[0, 0], p[2, 1] - p[0, 1], p[2, 2] - p[0, 2]
    a, b, c = b1 * c2 - b2 * c1, a2 * c1 - a1 * c2, a1 * b2 - b1 * a2
    d = (- a * p[0, 0] - b * p[0, 1] - c * p[0, 2])
    return -1 * np.array([a, b, c, d])


def _rodrigues(r):
    """cv2.Rodrigues(rotation vector) -> 3x3 matrix: cos I + (1 - cos) k k^T + sin [k]x."""
    r = np.asarray(r, np.float64).reshape(3)
    theta = math.sqrt(float(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
    if theta < 2.220446049250313e-16:
        return np.eye(3)
    k = r / theta
    c, s = math.cos(theta), math.sin(theta)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * kx


def _box_corners_camera(dim, location, rotation_y, denorm):
    """compute_box_3d_camera_v2: the box on the ground plane ``denorm`` -> [3, 8] camera-frame corners."""
    c, s = np.cos(rotation_y), np.sin(rotation_y)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float32)
    l, w, h = dim[2], dim[1], dim[0]
    corners = np.array([[l/2, l/2, -l/2, -l/2, l/2, l/2, -l/2, -l/2], [0, 0, 0, 0, -h, -h, -h, -h],
                        [w/2, -w/2, -w/2, w/2, w/2, -w/2, -w/2, w/2]], dtype=np.float32)
    corners = np.dot(R, corners)
    denorm = np.asarray(denorm, np.float64)[:3]
    unit = denorm / np.sqrt(denorm[0]**2 + denorm[1]**2 + denorm[2]**2)
    up = np.array([0.0, -1.0, 0.0])
    theta = -1 * math.acos(np.dot(unit, up))
    n = np.cross(denorm, up)
    n = n / np.sqrt(n[0]**2 + n[1]**2 + n[2]**2)
    corners = np.dot(_rodrigues(theta * n), corners)
    return corners + np.array(location, dtype=np.float32).reshape(3, 1)


def load_sample(calib_txt, label_txt, is_pred=False):
    """``load_calib_v2`` + ``load_annos`` + ``annos_cam2ego`` of one frame's calib and label files -> dict(Tr_ego2cam [4, 4],
    P2 [3, 4], denorm [4], objects).  Labels beyond 140 m, with unknown names, with zero size, and pseudo labels
    (``is_pred``: a 16th column) below 0.70 are dropped, as the reference drops them."""
    P2 = Tr = None
    with open(calib_txt, 'r') as fp:
        for row in csv.reader(fp, delimiter=' '):
            if row and row[0] == 'P2:':
                P2 = np.array([float(i) for i in row[1:]], dtype=np.float32).reshape(3, 4)
            elif row and row[0] == 'Tr_velo_to_cam:':
                Tr = np.array([float(i) for i in row[1:]], dtype=np.float32).reshape(3, 4)
    if P2 is None or Tr is None:
        raise ValueError(f"{calib_txt}: no P2 / Tr_velo_to_cam line")
    Tr = np.concatenate((Tr, np.array([[0, 0, 0, 1]])), axis=0)
    Tr_cam2ego = np.linalg.inv(Tr)
    Tr_ego2cam = np.linalg.inv(Tr_cam2ego)
    denorm = get_denorm(Tr_ego2cam)
    obj = dict(corners=[], dim=[], truncated=[], occluded=[], score=[], names=[])
    with open(label_txt, 'r') as fp:
        for row in csv.reader(fp, delimiter=' '):
            if not row:
                continue
            loc = np.array((float(row[11]), float(row[12]), float(row[13])), dtype=np.float32)
            if math.sqrt(loc[0]**2 + loc[1]**2 + loc[2]**2) > 140:
                continue
            if row[0].lower() not in NAMES:
                continue
            dim = [float(row[8]), float(row[9]), float(row[10])]
            if sum(dim) == 0:
                continue
            score = float(row[15]) if is_pred else 1.0
            if score < 0.70:
                continue
            cam = _box_corners_camera(np.array(dim).astype(float), loc.astype(float), float(row[14]), denorm)
            cam = np.concatenate((cam, np.ones((1, 8))), axis=0)
            obj['corners'].append(np.matmul(Tr_cam2ego, cam)[:3, :])
            obj['dim'].append(dim)
            obj['truncated'].append(float(row[1]))
            obj['occluded'].append(float(row[2]))
            obj['score'].append(score)
            obj['names'].append(row[0])
    n = len(obj['names'])
    objects = dict(corners=np.array(obj['corners'], np.float64).reshape(n, 3, 8), dim=np.array(obj['dim'], np.float64).reshape(n, 3),
                   truncated=np.array(obj['truncated'], np.float64), occluded=np.array(obj['occluded'], np.float64),
                   score=np.array(obj['score'], np.float64), names=obj['names'])
    return dict(Tr_ego2cam=Tr_ego2cam, P2=P2, denorm=denorm, objects=objects)


def empty_objects():
    return dict(corners=np.zeros((0, 3, 8)), dim=np.zeros((0, 3)), truncated=np.zeros(0), occluded=np.zeros(0), score=np.zeros(0),
                names=[])


def pack_objects(objects, order=None):
    """-> (f64 [n, 30] rows of the C ABI, i32 [n] classes, names) of one frame's objects, in ``order`` if given."""
    n = len(objects['names'])
    idx = np.arange(n) if order is None else np.asarray(list(order), np.int64).reshape(-1)
    rows = np.empty((len(idx), OBJ_COLS), np.float64)
    rows[:, :24] = np.asarray(objects['corners'], np.float64).reshape(n, 24)[idx]
    rows[:, 24:27] = np.asarray(objects['dim'], np.float64).reshape(n, 3)[idx]
    for k, key in enumerate(('truncated', 'occluded', 'score')):
        rows[:, 27 + k] = np.asarray(objects[key], np.float64).reshape(n)[idx]
    names = [objects['names'][i] for i in idx]
    low = [s.lower() for s in names]
    unknown = [s for s in low if s not in NAMES]
    if unknown:
        raise ValueError(f"unknown object names {sorted(set(unknown))}: filter them as load_annos does")
    return rows, np.array([NAMES.index(s) for s in low], np.int32), names


def frame_descriptors(dest, sources, index_of, order=None, rng=None):
    """The descriptors and object arrays of a batch.  ``dest``: B frames, ``sources``: B lists of at most three frames;
    ``index_of(frame)``: its pool index.  ``order``: per frame, per source, a permutation (or subset) of that source's
    objects; without it ``rng`` (a ``random.Random``) draws one as the reference does (``draw_order``), and without either the objects keep
    their order.  -> (descriptors [B], objects f64 [n, 30], classes i32 [n], names per frame)."""
    B = len(dest)
    assert B >= 1 and len(sources) == B
    desc = np.zeros(B, FRAME_DTYPE)
    rows, classes, names = [], [], []
    total = 0
    for b in range(B):
        d, srcs = dest[b], list(sources[b])
        if len(srcs) > MAX_SOURCES:
            raise ValueError(f"frame {b}: {len(srcs)} sources, at most {MAX_SOURCES}")
        Tr, P2 = np.asarray(d['Tr_ego2cam'], np.float64), np.asarray(d['P2'], np.float64)
        f = desc[b]
        f['dest'], f['n_src'], f['obj0'] = index_of(d), len(srcs), total
        f['tr'], f['p2'] = Tr[:3, :4].reshape(-1), P2[:3, :4].reshape(-1)
        r, c, nm = pack_objects(d.get('objects') or empty_objects())
        parts, frame_names = [(r, c)], list(nm)
        f['n_obj'][0] = len(c)
        for s, src in enumerate(srcs):
            Ts = np.asarray(src['Tr_ego2cam'], np.float64)
            f['src'][s] = index_of(src)
            f['minv'][s] = homography(Ts, src['P2'], Tr, P2)[1].reshape(-1)
            f['delta'][s] = np.linalg.inv(Tr)[:3, 3] - np.linalg.inv(Ts)[:3, 3]
            obj = src.get('objects') or empty_objects()
            if order is not None:
                perm = order[b][s]
            elif rng is not None:
                perm = draw_order(obj, rng, _in_view(obj['corners'], f['delta'][s], Tr, P2))
            else:
                perm = None
            r, c, nm = pack_objects(obj, perm)
            parts.append((r, c))
            frame_names += nm
            f['n_obj'][1 + s] = len(c)
        total += len(frame_names)
        rows += [p[0] for p in parts]
        classes += [p[1] for p in parts]
        names.append(frame_names)
    return desc, np.concatenate(rows).reshape(-1, OBJ_COLS), np.concatenate(classes).astype(np.int32), names


def label_lines(names, rows, info):
    """Label text of one generated frame from the kernel's rows [m, 15] and row_info [m, 2]."""
    lines = []
    for r, (j, clamped) in zip(np.asarray(rows).tolist(), np.asarray(info).tolist()):
        f = [repr(v) for v in r[2:]]
        if clamped & 1:
            f[1] = "0"                                        # Python's max(0, xmin) returned the integer
        if clamped & 2:
            f[2] = "0"
        lines.append(" ".join([names[j], str(r[0]), str(r[1])] + f))
    return lines


class RecombineResult:
    """``frames`` u8 [B, H, W, 3] and ``masks`` u8 [B, H, W] are on the device and ordered on the stream they were made on;
    ``labels()`` waits for the one copy that brings everything else to pinned memory."""

    def __init__(self, frames, masks, host, event, layout, names, max_obj):
        self.frames, self.masks = frames, masks
        self._host, self._event, self._layout, self._names, self._max_obj = host, event, layout, names, max_obj
        self._labels = None

    def mask_image(self):
        """The masks as the dataset stores them and ``TrainAugmenter.mask`` / ``ImagePreprocessor.mask`` take them: ids x 40,
        u8 [B, H, W, 1]."""
        return (self.masks * 40).unsqueeze(-1)

    def labels(self):
        """-> per generated frame a dict: ``lines`` (label text), ``names``, ``rows`` f64 [m, 15], ``beta`` [3], ``kept`` (flag
        per input object, the destination's first) and ``boxes`` f64 [n, 4] (the float 2-D box of every input object)."""
        if self._labels is None:
            self._event.synchronize()
            buf, (o_beta, o_boxes, o_kept, o_n, o_rows, o_info, _), M = self._host.numpy(), self._layout, self._max_obj
            B = len(self._names)
            beta = buf[o_beta:o_beta + B * 24].view(np.float64).reshape(B, 3)
            boxes = buf[o_boxes:o_boxes + B * M * 32].view(np.float64).reshape(B, M, 4)
            kept = buf[o_kept:o_kept + B * M * 4].view(np.int32).reshape(B, M)
            n_rows = buf[o_n:o_n + B * 4].view(np.int32)
            rows = buf[o_rows:o_rows + B * M * ROW_COLS * 8].view(np.float64).reshape(B, M, ROW_COLS)
            info = buf[o_info:o_info + B * M * 8].view(np.int32).reshape(B, M, 2)
            out = []
            for b, names in enumerate(self._names):
                m, n = int(n_rows[b]), len(names)
                out.append(dict(lines=label_lines(names, rows[b, :m], info[b, :m]), names=[names[j] for j in info[b, :m, 0]],
                                rows=rows[b, :m].copy(), beta=beta[b].copy(), kept=kept[b, :n].astype(bool), boxes=boxes[b, :n].copy()))
            self._labels = out
        return self._labels


class FrameRecombiner:
    def __init__(self, src_hw=(1080, 1920), max_sources=3, max_obj=256):
        self.H, self.W = int(src_hw[0]), int(src_hw[1])
        self.max_sources, self.max_obj = int(max_sources), int(max_obj)
        if not (1 <= self.max_sources <= MAX_SOURCES):
            raise ValueError(f"max_sources is 1..{MAX_SOURCES}, not {max_sources}")
        if self.H < 2 or self.W < 2 or self.max_obj < 1:
            raise ValueError("frames are at least 2 x 2 and max_obj at least 1")

    def _layout(self, B):
        M, o, offs = self.max_obj, 0, []
        for nbytes in (B * 24, B * M * 32, B * M * 4, B * 4, B * M * ROW_COLS * 8, B * M * 8):
            offs.append(o)
            o += _up(nbytes)
        return tuple(offs) + (o,)

    def combine(self, dest, sources, order=None, rng=None, pool=None):
        """``dest``: B frames, ``sources``: per frame its ordered list of at most ``max_sources`` frames.  A frame is a dict:
        ``image`` u8 [H, W, 3] RGB and ``mask`` u8 [H, W] class ids on the device (or, with ``pool=(images [N, H, W, 3],
        masks [N, H, W])``, ``index`` into the pool), ``Tr_ego2cam`` [4, 4], ``P2`` [3, 4] and ``objects`` as ``load_sample``
        returns them.  ``order`` / ``rng``: see ``frame_descriptors``.  Everything is enqueued on the current stream."""
        import torch
        lib = _lib.load()
        B = len(dest)
        for b, srcs in enumerate(sources):
            if len(srcs) > self.max_sources:
                raise ValueError(f"frame {b}: {len(srcs)} sources, max_sources is {self.max_sources}")
        if pool is None:
            frames, slot = [], {}

            def index_of(fr):
                if id(fr) not in slot:
                    slot[id(fr)] = len(frames)
                    frames.append(fr)
                return slot[id(fr)]
        else:
            def index_of(fr):
                return int(fr['index'])
        desc, objects, classes, names = frame_descriptors(dest, sources, index_of, order, rng)
        for b in range(B):
            n = int(desc[b]['n_obj'].sum())
            if n > self.max_obj:
                raise ValueError(f"frame {b}: {n} objects, max_obj is {self.max_obj}")
        if pool is None:
            images = torch.stack([f['image'] for f in frames])
            masks = torch.stack([f['mask'] for f in frames])
        else:
            images, masks = pool
        if not (images.is_cuda and masks.is_cuda):
            raise RuntimeError("FrameRecombiner.combine: frames and masks must be on the GPU (there is no CPU path)")
        N = images.shape[0]
        assert images.dtype == torch.uint8 and masks.dtype == torch.uint8 and images.is_contiguous() and masks.is_contiguous()
        assert tuple(images.shape) == (N, self.H, self.W, 3) and tuple(masks.shape) == (N, self.H, self.W), \
            f"frames {tuple(images.shape)} / masks {tuple(masks.shape)} are not [{N}, {self.H}, {self.W}, 3] / [{N}, {self.H}, {self.W}]"
        dev, M = images.device, self.max_obj
        n_obj = len(classes)
        # one upload: descriptors | objects | classes
        o_obj = _up(B * FRAME_DTYPE.itemsize)
        o_cls = o_obj + _up(max(n_obj, 1) * OBJ_COLS * 8)
        up_bytes = o_cls + _up(max(n_obj, 1) * 4)
        layout = self._layout(B)
        host_in = torch.empty(up_bytes, dtype=torch.uint8).pin_memory()
        stage = host_in.numpy()
        stage[:B * FRAME_DTYPE.itemsize] = desc.view(np.uint8).reshape(-1)
        stage[o_obj:o_obj + n_obj * OBJ_COLS * 8] = objects.view(np.uint8).reshape(-1)
        stage[o_cls:o_cls + n_obj * 4] = classes.view(np.uint8).reshape(-1)
        nws = lib.sgv3d_recombine_workspace_bytes(B, self.H, self.W, M)
        if nws == 0:
            raise _lib.SGV3DError("sgv3d_recombine_workspace_bytes refused the sizes")
        with torch.cuda.device(dev):
            din = torch.empty(up_bytes, dtype=torch.uint8, device=dev)
            din.copy_(host_in, non_blocking=True)
            dout = torch.empty(layout[-1], dtype=torch.uint8, device=dev)
            work = torch.empty(nws, dtype=torch.uint8, device=dev)
            out_images = torch.empty(B, self.H, self.W, 3, dtype=torch.uint8, device=dev)
            out_masks = torch.empty(B, self.H, self.W, dtype=torch.uint8, device=dev)
            p_in, p_out = din.data_ptr(), dout.data_ptr()
            rc = lib.sgv3d_recombine_frames(
                B, N, self.H, self.W, M, n_obj, desc.ctypes.data_as(ctypes.c_void_p), p_in, images.data_ptr(), masks.data_ptr(),
                p_in + o_obj, p_in + o_cls, work.data_ptr(), nws, out_images.data_ptr(), out_masks.data_ptr(), p_out + layout[0],
                p_out + layout[1], p_out + layout[2], p_out + layout[3], p_out + layout[4], p_out + layout[5], _lib.stream_handle(dev))
            _lib.check(rc, "sgv3d_recombine_frames")
            host = torch.empty(layout[-1], dtype=torch.uint8).pin_memory()
            host.copy_(dout, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        del host_in, din, dout, work        # the caching allocators keep them alive for work already enqueued on this stream
        return RecombineResult(out_images, out_masks, host, ev, layout, names, M)


def write(root, frame_id, image, mask, dest, lines, img_path="training/image_2", encoded=None):
    """``save_kitti_format`` of one generated frame: ``calib``, ``denorm``, ``label_2`` and ``mask_image`` (ids x 40, three
    channels, .npy) under ``root/training`` and the image under ``root/img_path`` (written through Pillow: the encoded
    bytes are Pillow's, not OpenCV's).  ``image`` u8 [H, W, 3] RGB and ``mask`` u8 [H, W] are host arrays or tensors;
    ``dest`` carries the generated frame's ``Tr_ego2cam`` and ``P2``.  ``encoded``: the frame's JPEG file as bytes (one of
    ``JpegEncoder(...)(frames).files()``): written as the .jpg as it is, and ``image`` is neither downloaded nor encoded
    here (it may be None)."""
    if encoded is None:
        from PIL import Image
        image = np.asarray(image.cpu() if hasattr(image, 'cpu') else image)
    elif not isinstance(encoded, (bytes, bytearray, memoryview)) or bytes(encoded[:2]) != b'\xff\xd8':
        raise ValueError("write: encoded must be the bytes of a JPEG file")
    mask = np.asarray(mask.cpu() if hasattr(mask, 'cpu') else mask)
    for sub in ("denorm", "calib", "label_2", "mask_image"):
        os.makedirs(os.path.join(root, "training", sub), exist_ok=True)
    os.makedirs(os.path.join(root, img_path), exist_ok=True)
    np.save(os.path.join(root, "training", "mask_image", frame_id + ".npy"), np.repeat(mask[:, :, None], 3, axis=2) * 40)
    if encoded is None:
        Image.fromarray(image).save(os.path.join(root, img_path, frame_id + ".jpg"))
    else:
        with open(os.path.join(root, img_path, frame_id + ".jpg"), "wb") as fp:
            fp.write(encoded)
    Tr = np.asarray(dest['Tr_ego2cam'])
    with open(os.path.join(root, "training", "calib", frame_id + ".txt"), "w") as fp:
        for key, val in (("P0", np.zeros((3, 4))), ("P1", np.zeros((3, 4))), ("P2", np.asarray(dest['P2'])), ("Tr_velo_to_cam", Tr[:3, :4])):
            fp.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in val.flatten())))
    with open(os.path.join(root, "training", "denorm", frame_id + ".txt"), "w") as fp:
        fp.write(" ".join(str(item) for item in get_denorm(Tr)) + "\n")
    with open(os.path.join(root, "training", "label_2", frame_id + ".txt"), "w") as fp:
        for line in lines:
            fp.write(line + "\n")
