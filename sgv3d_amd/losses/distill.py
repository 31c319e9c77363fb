"""``EmbedDistillation``: ``F.mse_loss(gt_embeds, assist_features) * weight`` of the reference's experiment file
(exps/bevheight/dair-v2x/bev_height_lss_r50_864_1536_128x128.py:247-256) on the MI355X (csrc/embed_distill.hip), with the
dataset's embedding warp (dataset/nusc_mv_det_dataset.py:351-385) folded in: the warped teacher is formed per pixel and never
written.  The forward is two launches (per-workgroup float64 partials over a fixed grid, a one-workgroup finish), the backward
one launch that recomputes the warp; sums are added in a fixed order, so a value and a gradient are bitwise repeatable, and
nothing waits on the host, so forward + backward capture into the training step's hipGraph.

``forward(assist, teacher, minv=None, warped=None)``:

* ``assist`` float32 [B, C, h, w], read in place through its strides: the NCHW view of the NHWC buffer that
  ``train_forward.bevheight_train_forward`` hands out under ``is_train_height``, a plain NCHW tensor, a batch slice;
* ``teacher`` float32 [B, h, w, C] NHWC (``distill.SamTeacher``); it never gets a gradient;
* ``minv`` [B, 3, 3] float64 and ``warped`` [B] from ``distill.embed_warp_matrices``: frame b with ``warped[b] != 0`` is
  compared with the teacher warped by ``minv[b]``, any other frame with the teacher as it is.  Without them the result is plain
  ``weight * mse``.  Host arrays are uploaded on every call; pass device tensors inside a graph capture.

``mask_dead=False`` is the reference's composition: a pixel whose source lies outside the teacher's frame has target 0 and
counts.  With ``mask_dead=True`` those pixels leave both the sum and the element count (counted on the device); a frame
without a live pixel contributes nothing, and with no live pixel at all loss and gradient are 0.

CPU tensors, non-float32 inputs, shape mismatches and shapes outside ``hip_ops.embed_distill_covers`` raise before any launch.
"""
import torch
from torch.nn.modules.loss import _Loss

from .. import _lib, hip_ops
from ..distill import device_matrices
from ..hip_ops import prof

__all__ = ['EmbedDistillation']


class _Distill(torch.autograd.Function):
    """``cfg`` = ((B, C, h, w, sb, sc, sp), weight, mask_dead)."""

    @staticmethod
    def forward(ctx, assist, teacher, minv, warped, cfg):
        (b, c, h, w, sb, sc, sp), weight, mask_dead = cfg
        lib = _lib.load()
        dev = assist.device
        nws = lib.sgv3d_embed_distill_workspace_bytes()
        ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        saved = torch.empty(2, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev), prof("embed_distill"):
            rc = lib.sgv3d_embed_distill_forward(b, c, h, w, assist.data_ptr(), sb, sc, sp, teacher.data_ptr(), _lib.ptr(minv),
                                                 _lib.ptr(warped), float(weight), 1 if mask_dead else 0, out.data_ptr(),
                                                 saved.data_ptr(), ws.data_ptr(), nws, _lib.stream_handle(dev))
        _lib.check(rc, "sgv3d_embed_distill_forward")
        ctx.cfg = cfg
        ctx.has_matrices = minv is not None
        if minv is None:
            ctx.save_for_backward(assist, teacher, saved)      # two numbers, not a gradient tensor
        else:
            ctx.save_for_backward(assist, teacher, saved, minv, warped)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        assist, teacher, saved = ctx.saved_tensors[:3]
        minv, warped = ctx.saved_tensors[3:] if ctx.has_matrices else (None, None)
        (b, c, h, w, sb, sc, sp), _, mask_dead = ctx.cfg
        dev = assist.device
        up = g.to(torch.float32).contiguous()           # stays on the device: the kernel reads the upstream scalar itself
        grad = torch.empty_strided(assist.size(), assist.stride(), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), prof("embed_distill_backward"):
            rc = _lib.load().sgv3d_embed_distill_backward(b, c, h, w, assist.data_ptr(), sb, sc, sp, teacher.data_ptr(),
                                                          _lib.ptr(minv), _lib.ptr(warped), 1 if mask_dead else 0,
                                                          saved.data_ptr(), up.data_ptr(), grad.data_ptr(),
                                                          _lib.stream_handle(dev))
        _lib.check(rc, "sgv3d_embed_distill_backward")
        return grad, None, None, None, None


class EmbedDistillation(_Loss):
    def __init__(self, weight=1000.0, mask_dead=False):
        super().__init__()
        self.weight = float(weight)
        self.mask_dead = bool(mask_dead)

    def forward(self, assist, teacher, minv=None, warped=None):
        for name, t in (("assist", assist), ("teacher", teacher)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"EmbedDistillation: {name}: sgv3d_amd.losses runs on the MI355X only (no CPU fallback)")
            if t.dtype != torch.float32:
                raise TypeError(f"EmbedDistillation: {name} must be float32, got {t.dtype}")
        if assist.dim() != 4 or teacher.dim() != 4:
            raise ValueError(f"EmbedDistillation: assist [B, C, h, w] and teacher [B, h, w, C] expected, got "
                             f"{tuple(assist.shape)} and {tuple(teacher.shape)}")
        b, c, h, w = (int(s) for s in assist.shape)
        if tuple(teacher.shape) != (b, h, w, c):
            raise ValueError(f"EmbedDistillation: assist {tuple(assist.shape)} needs a teacher {(b, h, w, c)}, got "
                             f"{tuple(teacher.shape)}")
        if teacher.device != assist.device:
            raise ValueError(f"EmbedDistillation: assist on {assist.device}, teacher on {teacher.device}")
        if b == 0 or not hip_ops.embed_distill_covers(c, h, w):
            raise _lib.SGV3DError(f"EmbedDistillation: shape {tuple(assist.shape)} is not covered (hip_ops.embed_distill_covers)")
        if (minv is None) != (warped is None):
            raise ValueError("EmbedDistillation: minv and warped go together (distill.embed_warp_matrices returns both)")
        if minv is not None:
            minv, warped = device_matrices(minv, warped, b, assist.device)
        teacher = teacher.detach().contiguous()
        x = assist
        st = x.stride()
        if st[2] != st[3] * w or min(st[1:]) < 1:
            x = x.contiguous()                  # the two spatial dims must be one run of pixels; batch / channel strides are free
            st = x.stride()
        cfg = ((b, c, h, w, st[0], st[1], st[3]), self.weight, self.mask_dead)
        return _Distill.apply(x, teacher, minv, warped, cfg)
