"""float64 numpy restatement of the fused lift-splat and its adjoint (layers/backbones/lss_fpn.py:462-466,486 followed by
ops/voxel_pooling/voxel_pooling.py:58-69, the kept test of oracle/voxel_pooling_ref.c):

    out[b, y, x, :]      = sum over kept (d, p) with v(b, d, p) = (y, x) of prob[b, d, p] * context[b, p, :]
    grad_prob[b, d, p]   = sum_c context[b, p, c] * G[b, v(b, d, p), c]      (0 where the point is not kept)
    grad_context[b, p, c] = sum_d prob[b, d, p] * G[b, v(b, d, p), c]        (kept d only)

with the sums of absolute terms ``A_prob`` / ``A_ctx`` that the a-priori f32 error bounds are stated in."""
import numpy as np


def kept_mask(geom, voxel_num):
    """geom int [B, D*P, 3] -> bool [B, D*P]: 0 <= x < X, 0 <= y < Y, 0 <= z < Z (z is only bounds-checked)."""
    X, Y, Z = voxel_num
    x, y, z = geom[..., 0], geom[..., 1], geom[..., 2]
    return (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)


def forward(geom, prob, context, voxel_num):
    """-> out float64 [B, Y, X, C]"""
    X, Y, _ = voxel_num
    B, D, P = prob.shape
    C = context.shape[-1]
    geom = np.asarray(geom).reshape(B, D * P, 3)
    prob, context = np.asarray(prob, np.float64), np.asarray(context, np.float64)
    keep = kept_mask(geom, voxel_num)
    out = np.zeros((B, Y * X, C))
    for b in range(B):
        lifted = (prob[b][:, :, None] * context[b][None, :, :]).reshape(D * P, C)
        k = keep[b]
        np.add.at(out[b], geom[b, k, 1] * X + geom[b, k, 0], lifted[k])
    return out.reshape(B, Y, X, C)


def backward(geom, prob, context, grad_out, voxel_num):
    """grad_out [B, Y, X, C] -> dict(grad_prob [B, D, P], grad_context [B, P, C], A_prob, A_ctx), all float64."""
    X, Y, _ = voxel_num
    B, D, P = prob.shape
    C = context.shape[-1]
    geom = np.asarray(geom).reshape(B, D, P, 3)
    prob, context = np.asarray(prob, np.float64), np.asarray(context, np.float64)
    G = np.asarray(grad_out, np.float64).reshape(B, Y * X, C)
    keep = kept_mask(geom, voxel_num)                                   # [B, D, P]
    vox = np.where(keep, geom[..., 1] * X + geom[..., 0], 0)
    grad_prob, a_prob = np.zeros((B, D, P)), np.zeros((B, D, P))
    grad_ctx, a_ctx = np.zeros((B, P, C)), np.zeros((B, P, C))
    for b in range(B):
        for d in range(D):
            rows = G[b, vox[b, d]] * keep[b, d][:, None]                # [P, C], zero rows where the point is not kept
            t = context[b] * rows
            grad_prob[b, d] = t.sum(-1)
            a_prob[b, d] = np.abs(t).sum(-1)
            t = prob[b, d][:, None] * rows
            grad_ctx[b] += t
            a_ctx[b] += np.abs(t)
    return dict(grad_prob=grad_prob, grad_context=grad_ctx, A_prob=a_prob, A_ctx=a_ctx)
