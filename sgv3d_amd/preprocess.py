"""On-device image preprocessing: decoded uint8 camera frames -> the float32 images and ``ida_mats`` ``BEVHeight.forward`` takes.

Replaces the reference dataset's per-image CPU path (dataset/nusc_mv_det_dataset.py:133-161 ``img_transform``: PIL bicubic
``resize``, ``crop``, optional left-right flip; :594-625 ``mmcv.imnormalize(img, mean, std, to_rgb)`` and the HWC->CHW
permute; :603-614 the semantic mask through the same transform, ``(mask / 40).astype(uint8)[..., 0]``) with one HIP launch
per batch (csrc/preprocess.hip).  The resize is Pillow's 8-bit resampler restated bit for bit; the crop box and the
augmentation matrix are the evaluation-time ones of ``input_contract.ida_resize_crop`` / ``ida_matrix``.

    pre = ImagePreprocessor(ida_aug_conf, img_conf, src_hw=(1080, 1920))
    imgs, ida_mats = pre(frames)          # frames: uint8 cuda [B, H, W, 3] or [B, S, N, H, W, 3]
    preds = model(imgs, mats)             # mats['ida_mats'] = ida_mats (or pre.ida through collate_mats)

Nothing here synchronises the host: a call can be captured in a hipGraph (``FramePipeline(..., preprocess=pre)``).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .input_contract import ida_matrix, ida_resize_crop

__all__ = ['ImagePreprocessor', 'resample_coeffs']


def resample_coeffs(in_size, out_size):
    """Pillow's bicubic coefficients for one axis (host, ``sgv3d_resample_coeffs``): (bounds int32 [out, 2] = first input
    pixel and number of taps, coeffs int32 [out, ksize] with 22 fractional bits)."""
    lib = _lib.load()
    ks = ctypes.c_int()
    _lib.check(lib.sgv3d_resample_coeffs(int(in_size), int(out_size), None, None, ctypes.byref(ks)), "resample_coeffs")
    bounds = np.zeros((int(out_size), 2), np.int32)
    coeffs = np.zeros((int(out_size), ks.value), np.int32)
    _lib.check(lib.sgv3d_resample_coeffs(int(in_size), int(out_size), bounds.ctypes.data, coeffs.ctypes.data,
                                         ctypes.byref(ks)), "resample_coeffs")
    return bounds, coeffs


_TABLES = {}   # (in, out, device) -> (bounds, coeffs, ksize) on the device: uploaded once per size pair


def _device_tables(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    t = _TABLES.get(key)
    if t is None:
        b, c = resample_coeffs(in_size, out_size)
        t = _TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), c.shape[1])
    return t


class ImagePreprocessor:
    """uint8 camera frames of one source size -> (imgs float32 [B, S, N, 3, fH, fW], ida_mats float32 [B, S, N, 4, 4]).

    ``ida_aug_conf``: the experiment's dict ('final_dim', optional 'bot_pct_lim'); ``img_conf``: 'img_mean', 'img_std',
    'to_rgb'.  ``flip``: the left-right flip of ``img_transform``.  ``rotate``: only 0 (the reference never samples another
    value, dataset/...:433-446).  The tables and the augmentation matrix are built here, once."""

    def __init__(self, ida_aug_conf, img_conf, src_hw=(1080, 1920), flip=False, rotate=0.0, device=None):
        if rotate:
            raise NotImplementedError("ImagePreprocessor: ida rotation is not supported (the reference never samples one)")
        dev = torch.device(device if device is not None else 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev                                               # ('cpu': tables and matrices only, no calls)
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.final_dim = (int(ida_aug_conf['final_dim'][0]), int(ida_aug_conf['final_dim'][1]))
        self.flip = bool(flip)
        resize, (new_w, new_h), crop, _, _ = ida_resize_crop(self.src_hw, self.final_dim,
                                                             ida_aug_conf.get('bot_pct_lim', (0.0, 0.0)))
        self.resize, self.resize_dims, self.crop = resize, (new_w, new_h), tuple(int(v) for v in crop)
        self.ida = ida_matrix(resize, self.crop, self.flip, 0.0)        # what collate_mats takes as a camera's 'ida'
        self._ida_dev = torch.from_numpy(self.ida).to(self.device)
        mean = np.asarray(img_conf['img_mean'], np.float32).reshape(3)
        std = np.asarray(img_conf['img_std'], np.float32).reshape(3)
        self.to_rgb = bool(img_conf.get('to_rgb', False))
        self._mean = (ctypes.c_float * 3)(*mean.tolist())
        self._std = (ctypes.c_float * 3)(*std.tolist())
        H, W = self.src_hw
        self._x = _device_tables(W, new_w, self.device)
        self._y = _device_tables(H, new_h, self.device)

    def _check(self, t, what, channels=None):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"ImagePreprocessor: {what} must be a CUDA tensor")
        if t.dtype != torch.uint8:
            raise ValueError(f"ImagePreprocessor: {what} must be uint8, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"ImagePreprocessor: {what} must be contiguous")
        if t.device != self.device:
            raise ValueError(f"ImagePreprocessor: {what} is on {t.device}, built for {self.device}")
        hw = tuple(t.shape[-3:-1])
        if hw != self.src_hw:
            raise ValueError(f"ImagePreprocessor: {what} are {hw[0]}x{hw[1]}, built for {self.src_hw[0]}x{self.src_hw[1]}")
        if channels is not None and t.shape[-1] != channels:
            raise ValueError(f"ImagePreprocessor: {what} must have {channels} channels, got {t.shape[-1]}")

    def _geometry(self):
        (new_w, new_h), (cx, cy) = self.resize_dims, self.crop[:2]
        xb, xk, kx = self._x
        yb, yk, ky = self._y
        return (new_h, new_w, cx, cy, self.final_dim[0], self.final_dim[1], int(self.flip)), \
            (xb.data_ptr(), xk.data_ptr(), kx, yb.data_ptr(), yk.data_ptr(), ky)

    def __call__(self, frames, out=None):
        """frames uint8 cuda [B, H, W, 3] or [B, S, N, H, W, 3] (RGB, as PIL decodes) -> (imgs float32 [B, S, N, 3, fH, fW],
        ida_mats float32 [B, S, N, 4, 4]).  ``out``: an existing contiguous float32 tensor of that shape to write into."""
        self._check(frames, "frames", 3)
        if frames.dim() == 4:
            lead = (frames.shape[0], 1, 1)
        elif frames.dim() == 6:
            lead = tuple(frames.shape[:3])
        else:
            raise ValueError(f"ImagePreprocessor: frames must be [B, H, W, 3] or [B, S, N, H, W, 3], got {tuple(frames.shape)}")
        fH, fW = self.final_dim
        shape = lead + (3, fH, fW)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"ImagePreprocessor: out must be a contiguous float32 {shape} tensor on {self.device}")
        n = lead[0] * lead[1] * lead[2]
        H, W = self.src_hw
        geo, tabs = self._geometry()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sgv3d_preprocess_images(n, H, W, *geo, int(self.to_rgb), *tabs, self._mean, self._std,
                                                          frames.data_ptr(), out.data_ptr(), _lib.stream_handle(self.device)),
                       "preprocess_images")
        return out, self._ida_dev.expand(lead + (4, 4)).clone()

    def mask(self, masks):
        """Semantic masks uint8 cuda [B, H, W, C] or [B, N, H, W, C] -> gt_semantic uint8 [B, N, fH, fW] (channel 0, same
        resize / crop / flip, then // 40)."""
        self._check(masks, "masks")
        if masks.dim() == 4:
            lead = (masks.shape[0], 1)
        elif masks.dim() == 5:
            lead = tuple(masks.shape[:2])
        else:
            raise ValueError(f"ImagePreprocessor: masks must be [B, H, W, C] or [B, N, H, W, C], got {tuple(masks.shape)}")
        out = torch.empty(lead + self.final_dim, dtype=torch.uint8, device=self.device)
        H, W = self.src_hw
        geo, tabs = self._geometry()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sgv3d_preprocess_mask(lead[0] * lead[1], H, W, int(masks.shape[-1]), *geo, *tabs,
                                                        masks.data_ptr(), out.data_ptr(), _lib.stream_handle(self.device)),
                       "preprocess_mask")
        return out
