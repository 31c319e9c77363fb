"""Training-time camera augmentation on the device: the reference dataset's ``is_train`` image path
(dataset/nusc_mv_det_dataset.py get_image).

Per camera and sweep the reference draws, in this order (:550, :295-297 and :400-431, :618-619):

* ``random.random() < 0.5``: intrinsic / extrinsic rectification.  ``ratio ~ N(1, 0.2)`` rescales the focal lengths,
  ``roll ~ N(0, 2 deg)`` then ``pitch ~ N(0, 0.67 deg)`` rotate ego -> sensor; the frame is Lanczos-resized by ``ratio``,
  pasted into / cropped to its own size about the principal point, and rotated by ``-roll`` about it with a vertical
  translate ``transform_pitch`` (:94-110 img_intrin_extrin_transform).  The semantic mask follows (:553-554).
* ``random.random() < 0.3``: brightness jitter after the eval resize + crop, then ``random.random()`` for its size
  (:618-623).

``sample_params`` makes those draws; ``augment_camera`` applies the rectification to a camera's matrices on the host (numpy
on 4x4 matrices, as the reference does) and records each frame's principal point and ``transform_pitch``;
``TrainAugmenter`` turns uint8 frames into the model's float32 input on the device (csrc/augment.hip), bit for bit what
Pillow, OpenCV's 8-bit rules and mmcv make of them.

    rs, nps = random.Random(seed), np.random.RandomState(seed)
    params = sample_params(n, rs, nps)
    cams = [augment_camera(cam, params, i) for i, cam in enumerate(cameras)]
    aug = TrainAugmenter(ida_aug_conf, img_conf, src_hw=(1080, 1920))
    imgs, ida_mats = aug(frames, params)           # frames: uint8 cuda [B, H, W, 3] or [B, S, N, H, W, 3]
    gt_semantic = aug.mask(masks, params)
    mats = collate_mats([dict(c, ida=aug.ida) for c in cams], device)

Nothing here synchronises the host: per-frame descriptors and coefficient tables travel through one pinned host tensor and
a non-blocking copy on the current stream.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .preprocess import ImagePreprocessor

__all__ = ['AugmentParams', 'sample_params', 'rectify', 'augment_camera', 'rotate_matrix', 'scale_offsets',
           'resample_coeffs_filter', 'TrainAugmenter', 'FILTER_BICUBIC', 'FILTER_LANCZOS']

FILTER_BICUBIC, FILTER_LANCZOS = 0, 1
RATIO_RANGE, ROLL_RANGE, PITCH_RANGE = (1.0, 0.20), (0.0, 2.00), (0.0, 0.67)   # dataset/...:295-297

# mirror of sgv3d_aug_frame (include/sgv3d_hip.h)
FRAME_DTYPE = np.dtype({'names': ['ie', 'bright', 'rs_w', 'rs_h', 'off_x', 'off_y', 'kx', 'ky', 'xtab', 'ytab', 'slot',
                                  'pad', 'affine', 'u'],
                        'formats': ['<i4'] * 8 + ['<i8', '<i8', '<i4', '<i4', ('<f8', (6,)), '<f8'],
                        'offsets': [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 104], 'itemsize': 112})


@dataclass
class AugmentParams:
    """Per-frame draws.  ``ie``: rectify; ``ratio``, ``roll_deg``, ``pitch_deg``: its draws (unused where ``ie`` is False);
    ``bright``: brightness jitter; ``u``: its draw.  ``center`` (int [n, 2], the principal point as the reference truncates
    it) and ``transform_pitch`` (int [n]) are filled by ``augment_camera``, or given here together."""
    ie: np.ndarray
    ratio: np.ndarray
    roll_deg: np.ndarray
    pitch_deg: np.ndarray
    bright: np.ndarray
    u: np.ndarray
    center: np.ndarray = None
    transform_pitch: np.ndarray = None

    def __post_init__(self):
        n = len(self.ie)
        placed = self.center is not None and self.transform_pitch is not None
        self.ie = np.asarray(self.ie, bool).reshape(n)
        self.bright = np.asarray(self.bright, bool).reshape(n)
        for k in ('ratio', 'roll_deg', 'pitch_deg', 'u'):
            setattr(self, k, np.asarray(getattr(self, k), np.float64).reshape(n))
        self.center = np.zeros((n, 2), np.int64) if self.center is None else np.asarray(self.center, np.int64)
        self.transform_pitch = np.zeros(n, np.int64) if self.transform_pitch is None else \
            np.asarray(self.transform_pitch, np.int64)
        self._placed = np.full(n, placed)   # center / transform_pitch given here or recorded by augment_camera

    def __len__(self):
        return len(self.ie)


def sample_params(n, py_random, np_random):
    """``n`` frames' draws in the reference's order: ``py_random.random() < 0.5``; if so ``np_random.normal`` for ratio,
    roll and pitch; ``py_random.random() < 0.3``; if so ``py_random.random()``.  Seeded like the reference's global
    ``random`` / ``np.random`` it gives the same sequence."""
    ie, ratio, roll, pitch, bright, u = [], [], [], [], [], []
    for _ in range(int(n)):
        e = py_random.random() < 0.5
        r = ro = p = 0.0
        if e:
            r = np_random.normal(*RATIO_RANGE)
            ro = np_random.normal(*ROLL_RANGE)
            p = np_random.normal(*PITCH_RANGE)
        b = py_random.random() < 0.3
        v = py_random.random() if b else 0.0
        ie.append(e), ratio.append(r), roll.append(ro), pitch.append(p), bright.append(b), u.append(v)
    return AugmentParams(ie, ratio, roll, pitch, bright, u)


def rectify(intrin, ego2sensor, ratio, roll_deg, pitch_deg):
    """``sample_intrin_extrin_augmentation`` (dataset/...:400-431) for given draws: (intrin float32 [4, 4], ego2sensor
    float32 [4, 4], transform_pitch int).  The dtypes follow the reference (float32 inputs, float64 rotations), and so do
    its quirks: no homogeneous divide of the projected centre, ``int()`` truncation."""
    K = np.asarray(intrin, np.float32)
    E = np.asarray(ego2sensor, np.float32)
    Kr = K.copy()
    Kr[:2, :2] = K[:2, :2] * float(ratio)              # (np.random.normal returns a Python float)
    r = roll_deg * np.pi / 180
    rot_roll = np.array([[math.cos(r), -math.sin(r), 0, 0], [math.sin(r), math.cos(r), 0, 0], [0, 0, 1, 0],
                         [0, 0, 0, 1]])
    E_roll = np.matmul(rot_roll, E)
    p = pitch_deg * np.pi / 180
    rot_pitch = np.array([[1, 0, 0, 0], [0, math.cos(p), -math.sin(p), 0], [0, math.sin(p), math.cos(p), 0],
                          [0, 0, 0, 1]])
    E_pitch = np.matmul(rot_pitch, E_roll)
    M = Kr[:3, :3] @ E_pitch[:3, :3]                                   # get_M(R, K, R_r, K_r) = K_r R_r R^-1 K^-1
    M = M @ np.linalg.inv(E_roll[:3, :3])
    M = M @ np.linalg.inv(Kr[:3, :3])
    center = Kr[:2, 2]
    center_ref = np.matmul(M, np.array([center[0], center[1], 1.0]).T)[:2]
    return Kr, E_pitch.astype(np.float32), int(center_ref[1] - center[1])


def augment_camera(camera, params, i=0):
    """A ``collate_mats`` camera dict (4x4 'sensor2ego', 'intrin', ...) after frame ``i``'s rectification: rectified
    'intrin' and 'sensor2ego', and 'sensor2sensor' = (keyego2keysensor of the unaugmented camera @ the augmented
    sensor2ego)^-1 (dataset/...:584-588 for one sweep).  sensor2virtual and the reference height follow in collate_mats.
    Records the frame's principal point and transform_pitch in ``params``.  A frame without rectification keeps its
    matrices (and 'sensor2sensor' is the identity)."""
    out = dict(camera)
    s2e = np.asarray(camera['sensor2ego'], np.float32)
    K = np.asarray(camera['intrin'], np.float32)
    tp = 0
    if params.ie[i]:
        e2s = np.linalg.inv(s2e)
        K, e2s_r, tp = rectify(K, e2s, params.ratio[i], params.roll_deg[i], params.pitch_deg[i])
        s2e_r = np.linalg.inv(e2s_r)
        out['intrin'] = K
        out['sensor2ego'] = s2e_r
        out['sensor2sensor'] = np.linalg.inv(e2s @ s2e_r).astype(np.float32)
    else:
        out['sensor2sensor'] = np.eye(4, dtype=np.float32)
    c = K[:2, 2].astype(np.int32)
    params.center[i] = (int(c[0]), int(c[1]))
    params.transform_pitch[i] = tp
    params._placed[i] = True
    out['center'] = (int(c[0]), int(c[1]))
    out['transform_pitch'] = tp
    return out


def scale_offsets(src_hw, ratio, center):
    """((resized W, H), (off_x, off_y)) of img_intrin_extrin_transform's resize + paste / crop (dataset/...:98-108): the
    canvas pixel (y, x) is the resized pixel (y + off_y, x + off_x), black outside it."""
    h, w = src_hw
    new_w, new_h = int(w * ratio), int(h * ratio)
    h_min = int(center[1] * abs(1.0 - ratio))
    w_min = int(center[0] * abs(1.0 - ratio))
    sgn = -1 if ratio <= 1.0 else 1
    return (new_w, new_h), (sgn * w_min, sgn * h_min)


def rotate_matrix(angle, center, translate):
    """The inverse affine coefficients ``PIL.Image.rotate(angle, center=center, translate=translate)`` hands to its
    transform (Pillow's Image.rotate: angle mod 360, cos / sin rounded to 15 digits, centre and translate folded in)."""
    angle = -math.radians(angle % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -center[0] - translate[0], -center[1] - translate[1]
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += center[0]
    m[5] += center[1]
    return m


def resample_coeffs_filter(filt, in_size, out_size):
    """Pillow's coefficients for one axis and filter (host, ``sgv3d_resample_coeffs_filter``): (bounds int32 [out, 2],
    coeffs int32 [out, ksize])."""
    lib = _lib.load()
    ks = ctypes.c_int()
    _lib.check(lib.sgv3d_resample_coeffs_filter(int(filt), int(in_size), int(out_size), None, None, ctypes.byref(ks)),
               "resample_coeffs_filter")
    bounds = np.zeros((int(out_size), 2), np.int32)
    coeffs = np.zeros((int(out_size), ks.value), np.int32)
    _lib.check(lib.sgv3d_resample_coeffs_filter(int(filt), int(in_size), int(out_size), bounds.ctypes.data,
                                                coeffs.ctypes.data, ctypes.byref(ks)), "resample_coeffs_filter")
    return bounds, coeffs


_LANCZOS = {}   # (in, out) -> flat int32 table (bounds then coeffs), ksize


def _lanczos_table(in_size, out_size):
    key = (int(in_size), int(out_size))
    t = _LANCZOS.get(key)
    if t is None:
        b, c = resample_coeffs_filter(FILTER_LANCZOS, in_size, out_size)
        t = _LANCZOS[key] = (np.concatenate([b.reshape(-1), c.reshape(-1)]), c.shape[1])
    return t


class TrainAugmenter:
    """uint8 frames of one source size + per-frame ``AugmentParams`` -> (imgs float32 [B, S, N, 3, fH, fW], ida_mats
    float32 [B, S, N, 4, 4]); ``.mask`` -> gt_semantic.  The eval-time resize + crop, its ``ida`` matrix and the
    normalisation are ``ImagePreprocessor``'s (no flip or rotation: the reference's training samples neither)."""

    def __init__(self, ida_aug_conf, img_conf, src_hw=(1080, 1920), device=None):
        self.pre = ImagePreprocessor(ida_aug_conf, img_conf, src_hw, device=device)
        self.device, self.src_hw, self.final_dim, self.ida = self.pre.device, self.pre.src_hw, self.pre.final_dim, \
            self.pre.ida

    def _frames(self, t, what, ranks, channels=None):
        self.pre._check(t, what, channels)
        if t.dim() not in ranks:
            raise ValueError(f"TrainAugmenter: {what} must have rank {' or '.join(map(str, ranks))}, got "
                             f"{tuple(t.shape)}")
        return tuple(t.shape[:t.dim() - 3])

    def plan(self, params, n, mask=False):
        """Host side of a call: (descriptors FRAME_DTYPE [n], Lanczos tables int32, rectified count).  Raises ValueError
        for parameters the reference could not apply (a resized size below one pixel) or that were never placed by
        ``augment_camera``."""
        if len(params) != n:
            raise ValueError(f"TrainAugmenter: {len(params)} parameter sets for {n} frames")
        H, W = self.src_hw
        rec = np.zeros(n, FRAME_DTYPE)
        tabs, off, slot = [], 0, 0
        for i in range(n):
            r = rec[i]
            r['bright'] = int(bool(params.bright[i]) and not mask)
            if r['bright']:
                if not math.isfinite(params.u[i]):
                    raise ValueError(f"TrainAugmenter: frame {i}: non-finite u")
                r['u'] = params.u[i]
            if not params.ie[i]:
                continue
            if not params._placed[i]:
                raise ValueError(f"TrainAugmenter: frame {i} is rectified but augment_camera has not placed it")
            ratio = float(params.ratio[i])
            if not math.isfinite(ratio):
                raise ValueError(f"TrainAugmenter: frame {i}: non-finite ratio")
            center = (int(params.center[i][0]), int(params.center[i][1]))
            (nw, nh), (ox, oy) = scale_offsets((H, W), ratio, center)
            if nw < 1 or nh < 1:
                raise ValueError(f"TrainAugmenter: frame {i}: ratio {ratio} resizes {H}x{W} to {nh}x{nw}; height and "
                                 f"width must be > 0")
            tx, kx = _lanczos_table(W, nw)
            ty, ky = _lanczos_table(H, nh)
            r['ie'], r['rs_w'], r['rs_h'], r['off_x'], r['off_y'], r['kx'], r['ky'] = 1, nw, nh, ox, oy, kx, ky
            r['xtab'], r['ytab'], r['slot'] = off, off + tx.size, slot
            off += tx.size + ty.size
            tabs += [tx, ty]
            r['affine'] = rotate_matrix(-float(params.roll_deg[i]), center, (0, int(params.transform_pitch[i])))
            slot += 1
        tables = np.concatenate(tabs).astype(np.int32) if tabs else np.zeros(0, np.int32)
        return rec, tables, slot

    def _upload(self, rec, tables):
        """One pinned host buffer (descriptors, then tables) and one non-blocking copy on the current stream; the caching
        host allocator keeps the pinned block until that copy has run."""
        nb = rec.nbytes + tables.nbytes
        host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
        h = host.numpy()
        h[:rec.nbytes] = rec.view(np.uint8)
        h[rec.nbytes:] = tables.view(np.uint8)
        dev = host.to(self.device, non_blocking=True)
        return dev, dev.data_ptr(), dev.data_ptr() + rec.nbytes

    def _run(self, src, params, n, mask, out):
        rec, tables, rectified = self.plan(params, n, mask)
        H, W = self.src_hw
        fH, fW = self.final_dim
        lib = _lib.load()
        nbytes = lib.sgv3d_augment_workspace_bytes(n, rectified, H, W, fH, fW, int(mask))
        (new_h, new_w, cx, cy, oh, ow, _), tabs = self.pre._geometry()
        with torch.cuda.device(self.device):
            dev, fr_dev, tab_dev = self._upload(rec, tables)
            work = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
            common = (rec.ctypes.data, fr_dev, tab_dev, int(tables.size), new_h, new_w, cx, cy, oh, ow)
            stream = _lib.stream_handle(self.device)
            if mask:
                rc = lib.sgv3d_augment_mask(n, H, W, int(src.shape[-1]), *common, *tabs, src.data_ptr(), work.data_ptr(),
                                            int(nbytes), out.data_ptr(), stream)
            else:
                rc = lib.sgv3d_augment_images(n, H, W, *common, int(self.pre.to_rgb), *tabs, self.pre._mean,
                                              self.pre._std, src.data_ptr(), work.data_ptr(), int(nbytes),
                                              out.data_ptr(), stream)
            _lib.check(rc, "augment_mask" if mask else "augment_images")
        return out

    def __call__(self, frames, params):
        """frames uint8 cuda [B, H, W, 3] or [B, S, N, H, W, 3] (RGB), params: one set per frame in that order ->
        (imgs float32 [B, S, N, 3, fH, fW], ida_mats float32 [B, S, N, 4, 4])."""
        lead = self._frames(frames, "frames", (4, 6), 3)
        lead = (lead[0], 1, 1) if len(lead) == 1 else lead
        n = lead[0] * lead[1] * lead[2]
        self.plan(params, n)                            # argument errors before any allocation or launch
        out = torch.empty(lead + (3,) + self.final_dim, dtype=torch.float32, device=self.device)
        self._run(frames, params, n, False, out)
        return out, self.pre._ida_dev.expand(lead + (4, 4)).clone()

    def mask(self, masks, params):
        """Semantic masks uint8 cuda [B, H, W, C] or [B, N, H, W, C] -> gt_semantic uint8 [B, N, fH, fW] (channel 0
        through the same rectification, resize and crop, then // 40).  Brightness draws do not apply to masks."""
        lead = self._frames(masks, "masks", (4, 5))
        lead = (lead[0], 1) if len(lead) == 1 else lead
        n = lead[0] * lead[1]
        self.plan(params, n, mask=True)
        out = torch.empty(lead + self.final_dim, dtype=torch.uint8, device=self.device)
        return self._run(masks, params, n, True, out)
