"""Distilling SAM's image embedding into the camera backbone: the teacher call and the embedding warp around
``losses.EmbedDistillation`` (csrc/embed_distill.hip).

The reference leaves three fragments of this: ``assist_layer`` (a 1x1 512 -> 256 convolution, 256 being SAM's ``out_chans``;
layers/backbones/lss_fpn.py:301,459,493-494), ``build_sam_vit_b(final_dim, downsample_factor, checkpoint)`` whose output is
exactly the grid of ``assist_features`` (layers/backbones/sam_encoder.py:117-122), the loss
``F.mse_loss(gt_embeds, assist_features) * 1000`` (exps/bevheight/dair-v2x/bev_height_lss_r50_864_1536_128x128.py:247-256), and
the dataset's ``get_M`` / ``transform_with_M_bilinear`` / ``mask_embed_intrin_extrin_transform``
(dataset/nusc_mv_det_dataset.py:343-398), which move a stored embedding into the camera the intrinsic / extrinsic augmentation
produced.  Its dataset never returns ``gt_embeds``; here the ends meet:

    teacher = SamTeacher(build_sam_vit_b(final_dim, 16).cuda(), ida_aug_conf)
    embeds = teacher(frames_u8)                                      # [B, h, w, 256], the unaugmented frames, once
    minv, warped = embed_warp_matrices(cameras, rectified, params, teacher.scale)
    loss = EmbedDistillation(1000.0)(assist, embeds, minv, warped)   # assist: the model's aux output under is_train_height
"""
import numpy as np
import torch

from . import _lib, hip_ops
from .hip_ops import prof
from .input_contract import ida_resize_crop
from .segment_anything import ops as sam_ops
from .segment_anything.transforms import ResizeLongestSide

__all__ = ['embed_warp_matrix', 'embed_warp_matrices', 'warp_embed', 'SamTeacher']


def embed_warp_matrix(K, R, K_r, R_r, scale):
    """``inv(M)`` float64 [3, 3] for one frame, on the host in float64: ``M = K_r' R_r R^-1 K'^-1`` is the reference's
    ``get_M(R, K, R_r, K_r)`` (dataset/nusc_mv_det_dataset.py:343-349) after rows 0-1 of both intrinsics were multiplied by
    ``scale``; ``K``, ``R`` are the camera's intrinsics and ego -> sensor rotation (3x3 or the upper-left of 4x4), ``K_r``,
    ``R_r`` the rectified ones.

    ``scale`` takes the intrinsics from the pixels of the source frame to the pixels of the embedding.  The reference's
    ``mask_embed_intrin_extrin_transform`` is the case ``scale = 1 / 16``: its stored embedding is 1/16 of the source frame.
    Here the embedding lives on the ``final_dim / downsample_factor`` grid of the model's input, which is the source frame
    after the ida resize, so ``scale = ida resize / downsample_factor`` (0.8 / 16 = 0.05 for the shipped 864 x 1536 configs
    on 1080 x 1920 frames; ``SamTeacher.scale``)."""
    K = np.array(np.asarray(K, np.float64)[:3, :3])
    K_r = np.array(np.asarray(K_r, np.float64)[:3, :3])
    K[:2, :] = K[:2, :] * float(scale)
    K_r[:2, :] = K_r[:2, :] * float(scale)
    R = np.asarray(R, np.float64)[:3, :3]
    R_r = np.asarray(R_r, np.float64)[:3, :3]
    M = np.matmul(K_r, R_r)
    M = np.matmul(M, np.linalg.inv(R))
    M = np.matmul(M, np.linalg.inv(K))
    return np.linalg.inv(M)


def embed_warp_matrices(cameras, rectified_cameras, params, scale):
    """(minv float64 [B, 3, 3], warped uint8 [B] = ``params.ie``) for a batch: ``cameras`` are the ``collate_mats`` camera dicts
    ('intrin', 'sensor2ego') before and ``rectified_cameras`` after ``train_augment.augment_camera``.  A frame that was not
    rectified gets the identity and ``warped = 0`` (the warp copies it; see ``warp_embed``)."""
    n = len(params)
    if len(cameras) != n or len(rectified_cameras) != n:
        raise ValueError(f"embed_warp_matrices: {len(cameras)} cameras, {len(rectified_cameras)} rectified, {n} draws")
    minv = np.tile(np.eye(3), (n, 1, 1))
    for i in range(n):
        if params.ie[i]:
            e2s = np.linalg.inv(np.asarray(cameras[i]['sensor2ego'], np.float64))
            e2s_r = np.linalg.inv(np.asarray(rectified_cameras[i]['sensor2ego'], np.float64))
            minv[i] = embed_warp_matrix(cameras[i]['intrin'], e2s, rectified_cameras[i]['intrin'], e2s_r, scale)
    return minv, np.asarray(params.ie, np.uint8)


def check_embedding(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: sgv3d_amd.distill runs on the MI355X only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: must be float32, got {t.dtype}")
    if t.dim() != 4:
        raise ValueError(f"{what}: [B, h, w, C] expected, got {tuple(t.shape)}")
    b, h, w, c = (int(s) for s in t.shape)
    if b == 0 or not hip_ops.embed_distill_covers(c, h, w):
        raise _lib.SGV3DError(f"{what}: shape {tuple(t.shape)} is not covered (hip_ops.embed_distill_covers)")
    return b, h, w, c


def device_matrices(minv, warped, batch, device):
    """(minv f64 [B, 9], warped u8 [B]) on ``device``; host arrays are uploaded (not inside a graph capture), device tensors
    are checked and taken as they are."""
    if not (isinstance(minv, torch.Tensor) and minv.is_cuda):
        minv = torch.from_numpy(np.ascontiguousarray(np.asarray(minv, np.float64))).to(device)
    if not (isinstance(warped, torch.Tensor) and warped.is_cuda):
        warped = torch.from_numpy(np.ascontiguousarray(np.asarray(warped).astype(np.uint8))).to(device)
    if minv.dtype != torch.float64 or minv.numel() != 9 * batch:
        raise ValueError(f"minv: float64 [{batch}, 3, 3] expected, got {minv.dtype} {tuple(minv.shape)}")
    if warped.dtype not in (torch.uint8, torch.bool) or warped.numel() != batch:
        raise ValueError(f"warped: uint8 [{batch}] expected, got {warped.dtype} {tuple(warped.shape)}")
    return minv.contiguous(), warped.contiguous()


def warp_embed(teacher, minv, warped, return_dead=False):
    """The reference's ``transform_with_M_bilinear`` for a batch of embeddings (``sgv3d_embed_warp``, one launch): teacher
    float32 [B, h, w, C] NHWC on the GPU, ``minv`` [B, 3, 3] float64 and ``warped`` [B] from ``embed_warp_matrices`` (host
    arrays or device tensors).  A frame with ``warped[b] == 0`` is copied unchanged: the reference only warps rectified frames,
    and its identity warp would zero the last row and column.  With ``return_dead`` also the uint8 [B, h, w] map of the pixels
    that read outside the source (their channels are 0).  ``EmbedDistillation`` does not need this call: it forms the warped
    teacher on the fly.  It serves users who store warped targets, and the tests."""
    b, h, w, c = check_embedding(teacher, "warp_embed: teacher")
    teacher = teacher.contiguous()
    minv, warped = device_matrices(minv, warped, b, teacher.device)
    out = torch.empty_like(teacher)
    dead = torch.empty(b, h, w, dtype=torch.uint8, device=teacher.device) if return_dead else None
    with torch.cuda.device(teacher.device), prof("embed_warp"):
        rc = _lib.load().sgv3d_embed_warp(b, h, w, c, teacher.data_ptr(), minv.data_ptr(), warped.data_ptr(), out.data_ptr(),
                                          _lib.ptr(dead), _lib.stream_handle(teacher.device))
    _lib.check(rc, "sgv3d_embed_warp")
    return (out, dead) if return_dead else out


class SamTeacher:
    """SAM's image encoder as the teacher: ``teacher(frames)`` with uint8 [B, H, W, 3] source frames on the GPU returns the
    float32 NHWC embedding [B, h, w, out_chans] on the ``final_dim // downsample_factor`` grid, under ``no_grad``.  The frames
    go through the Pillow-BILINEAR resize ``SamPredictor.set_image`` uses, to ``get_preprocess_shape(H, W, img_size)``, then
    ``encoder.forward`` (``hip_ops.VIT_BF16`` applies as anywhere else).  ``.scale`` is the intrinsic scale
    ``embed_warp_matrices`` needs.

    The grids line up only if the encoder's 576 x 1024 crop is the whole resized frame, the ida transform of the model's input
    is the whole frame too, and the encoder resizes to the model's feature grid: anything else raises here."""

    def __init__(self, encoder, ida_aug_conf, src_hw=(1080, 1920)):
        self.encoder = encoder
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.size = ResizeLongestSide.get_preprocess_shape(self.src_hw[0], self.src_hw[1], int(encoder.img_size))
        if self.size != (576, 1024):
            raise ValueError(f"SamTeacher: {self.src_hw} frames resize to {self.size}; the encoder crops 576 x 1024 "
                             "(layers/backbones/sam_encoder.py:117-122), so its embedding would not cover the frame")
        fH, fW = (int(v) for v in ida_aug_conf['final_dim'])
        resize, dims, crop, flip, rotate = ida_resize_crop(self.src_hw, (fH, fW), ida_aug_conf.get('bot_pct_lim', (0.0, 0.0)))
        if tuple(dims) != (fW, fH) or tuple(crop) != (0, 0, fW, fH) or flip or rotate:
            raise ValueError(f"SamTeacher: the ida transform must be the whole frame (resize dims {tuple(dims)}, crop "
                             f"{tuple(crop)} for final_dim {(fH, fW)}): the model's input and the teacher's would differ")
        down = fH // int(encoder.out_dim[0])
        if down <= 0 or tuple(encoder.out_dim) != (fH // down, fW // down):
            raise ValueError(f"SamTeacher: encoder.out_dim {tuple(encoder.out_dim)} is not final_dim // downsample_factor "
                             f"of {(fH, fW)}")
        self.downsample_factor = down
        self.scale = resize / down

    def __call__(self, frames):
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise RuntimeError("SamTeacher: the frames must be a tensor on the GPU (there is no CPU fallback)")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != self.src_hw + (3,):
            raise ValueError(f"SamTeacher: uint8 [B, {self.src_hw[0]}, {self.src_hw[1]}, 3] expected, got {frames.dtype} "
                             f"{tuple(frames.shape)}")
        with torch.no_grad():
            x = sam_ops.resize_bilinear_u8(frames.contiguous(), self.size)
            return self.encoder.forward(x).permute(0, 2, 3, 1)
