"""Restatement of the embedding distillation (csrc/embed_distill.hip) in torch, written from the description of the operation
and not from the kernels: the reference's ``get_M`` and ``transform_with_M_bilinear`` (dataset/nusc_mv_det_dataset.py:343-385)
and ``F.mse_loss(gt_embeds, assist_features) * weight``.  In float64 on the CPU it is the oracle of the tests (pinned to the
reference's own outputs by tests/golden/embed_distill.npz); with ``dtype=torch.float32`` on the GPU it is the baseline of
tools/embed_distill_bench.py."""
import numpy as np
import torch


def warp_matrix(K, R, K_r, R_r, scale):
    """inv(M), M = K_r' R_r R^-1 K'^-1 with rows 0-1 of both intrinsics multiplied by ``scale``; float64 [3, 3]."""
    K = np.array(K, np.float64)[:3, :3].copy()
    K_r = np.array(K_r, np.float64)[:3, :3].copy()
    K[:2, :] = K[:2, :] * scale
    K_r[:2, :] = K_r[:2, :] * scale
    R = np.array(R, np.float64)[:3, :3]
    R_r = np.array(R_r, np.float64)[:3, :3]
    M = np.matmul(K_r, R_r)
    M = np.matmul(M, np.linalg.inv(R))
    M = np.matmul(M, np.linalg.inv(K))
    return np.linalg.inv(M)


def positions(minv, h, w, device=None):
    """(u, v) float64 [h, w]: where output pixel (x, y) reads, the point (10x, 10y, 10) through ``minv``."""
    m = torch.as_tensor(np.asarray(minv, np.float64).reshape(9)).to(device)
    X = (torch.arange(w, dtype=torch.float64, device=device) * 10.0).view(1, w).expand(h, w)
    Y = (torch.arange(h, dtype=torch.float64, device=device) * 10.0).view(h, 1).expand(h, w)
    Z = 10.0
    a = (m[0] * X + m[1] * Y) + m[2] * Z
    b = (m[3] * X + m[4] * Y) + m[5] * Z
    c = (m[6] * X + m[7] * Y) + m[8] * Z
    return a / c, b / c


def warp(image, minv, dtype=torch.float64):
    """One frame: image [h, w, C] float32 tensor -> (warped [h, w, C] float32, dead bool [h, w]).  Positions are float64; the
    blends run in ``dtype`` (float64 is the operation; float32 is the bench's baseline)."""
    h, w, _ = image.shape
    u, v = positions(minv, h, w, image.device)
    dead = (u < 0) | (u > w - 2) | (v < 0) | (v > h - 2)
    u = u.clamp(0, w - 2)
    v = v.clamp(0, h - 2)
    c0 = torch.floor(u)
    r0 = torch.floor(v)
    ax0, ax1 = ((c0 + 1) - u).to(dtype)[..., None], (u - c0).to(dtype)[..., None]
    ay0, ay1 = ((r0 + 1) - v).to(dtype)[..., None], (v - r0).to(dtype)[..., None]
    r, c = r0.long(), c0.long()
    img = image.to(dtype)
    f1 = ax0 * img[r, c] + ax1 * img[r, c + 1]
    f2 = ax0 * img[r + 1, c] + ax1 * img[r + 1, c + 1]
    out = ay0 * f1 + ay1 * f2
    out = torch.where(dead[..., None], torch.zeros((), dtype=dtype, device=image.device), out)
    return out.to(torch.float32), dead


def warp_batch(teacher, minv, warped, dtype=torch.float64):
    """teacher [B, h, w, C] float32; frames with ``warped[b]`` false are copied and have no dead pixel."""
    outs, deads = [], []
    for b in range(teacher.shape[0]):
        if minv is not None and bool(warped[b]):
            o, d = warp(teacher[b], minv[b], dtype)
        else:
            o, d = teacher[b], torch.zeros(teacher.shape[1:3], dtype=torch.bool, device=teacher.device)
        outs.append(o)
        deads.append(d)
    return torch.stack(outs), torch.stack(deads)


def distill_loss(student, target, dead=None, weight=1000.0, mask_dead=False):
    """student [B, C, h, w] (any float dtype, may require grad); target [B, h, w, C] the warped teacher (float32 values);
    the loss in the student's dtype.  Without ``mask_dead`` this is ``F.mse_loss(target, student) * weight``; with it the
    dead pixels leave the sum and the count."""
    t = target.permute(0, 3, 1, 2).to(student.dtype)
    d2 = (student - t) ** 2
    if not mask_dead or dead is None:
        return d2.sum() / d2.numel() * weight
    live = (~dead)[:, None].to(student.dtype)
    n = float(live.sum()) * student.shape[1]
    if n == 0:
        return (student * 0).sum()
    return (d2 * live).sum() / n * weight
