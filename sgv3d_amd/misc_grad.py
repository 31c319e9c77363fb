"""Differentiable forms of the small layers of the training forward that ran as ATen operators in round 1: the stem's
max pooling, the ASPP image-pooling branch (global average + 1x1 convolution on a [B, C] vector) and the deformable
bilinear sampling of the DCN.  NHWC float32 on the MI355X; forward kernels in
csrc/misc_layers.hip, adjoints in csrc/train_misc.hip.  ``deform_conv3x3`` is the whole DCN of the mixed-precision step in one
launch with no tensor of the column size kept (csrc/dcn_fused_bf16.hip forward, csrc/dcn_grad.hip weight gradient)."""
import torch

from . import _lib, grad_slots, hip_ops
from .hip_ops import prof

__all__ = ['maxpool3x3s2', 'pooled_linear', 'deform_im2col3x3', 'deform_conv3x3', 'deform_conv3x3_covers',
           'deform_conv3x3_backward_weight']


def _st(t):
    return _lib.stream_handle(t.device)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, C = (int(v) for v in x.shape)
        oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(B, oh, ow, C, dtype=torch.float32, device=x.device)
        idx = torch.empty(B, oh, ow, C, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device), prof("maxpool3x3s2_train"):
            rc = _lib.load().sgv3d_maxpool3x3s2_train_forward(B, H, W, C, x.data_ptr(), y.data_ptr(), idx.data_ptr(), _st(x))
        _lib.check(rc, "sgv3d_maxpool3x3s2_train_forward")
        ctx.save_for_backward(idx)
        ctx.in_shape = (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        B, H, W, C = ctx.in_shape
        dy = dy.contiguous()
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=dy.device)
        with torch.cuda.device(dy.device), prof("maxpool3x3s2_backward"):
            rc = _lib.load().sgv3d_maxpool3x3s2_backward(B, H, W, C, idx.data_ptr(), dy.data_ptr(), dx.data_ptr(), _st(dy))
        _lib.check(rc, "sgv3d_maxpool3x3s2_backward")
        return dx


def maxpool3x3s2(x):
    """``nn.MaxPool2d(3, 2, 1)`` on an NHWC map (channels % 4 == 0)."""
    return _MaxPool.apply(x.contiguous())


class _PooledLinear(torch.autograd.Function):
    """y[b] = W @ mean_pixels(x[b]): AdaptiveAvgPool2d((1, 1)) + bias-free 1x1 Conv2d of the ASPP (lss_fpn.py:80-88)."""

    @staticmethod
    def forward(ctx, x, weight):
        B, H, W, C = (int(v) for v in x.shape)
        w2 = weight.reshape(weight.shape[0], -1).contiguous()
        pooled = hip_ops.global_avgpool(x)                                   # [B, C]
        y = hip_ops.dense(pooled, w2)                                        # [B, N]
        ctx.save_for_backward(pooled, w2)
        ctx.x_shape, ctx.w_shape = (B, H, W, C), tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        pooled, w2 = ctx.saved_tensors
        B, H, W, C = ctx.x_shape
        dy = dy.contiguous()
        N = int(w2.shape[0])
        dpooled = hip_ops.dense(dy, w2.t().contiguous())                     # [B, C]
        dw = torch.empty(N, C, dtype=torch.float32, device=dy.device)
        with torch.cuda.device(dy.device), prof("dense_backward_weight"):
            rc = _lib.load().sgv3d_dense_backward_weight(B, C, N, pooled.data_ptr(), dy.data_ptr(), dw.data_ptr(), _st(dy))
        _lib.check(rc, "sgv3d_dense_backward_weight")
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=dy.device)
        hip_ops.broadcast_channels((dpooled * (1.0 / (H * W))).contiguous(), dx)   # every pixel receives d pooled / (H W)
        return dx, dw.reshape(ctx.w_shape)


def pooled_linear(x, weight):
    """x NHWC [B, H, W, C], weight [N, C, 1, 1] -> [B, N] = weight @ mean over pixels."""
    return _PooledLinear.apply(x.contiguous(), weight)


class _DeformIm2col(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offset, groups):
        col = hip_ops.deform_im2col3x3(x, offset, groups)
        ctx.save_for_backward(x, offset)
        ctx.groups = groups
        return col

    @staticmethod
    def backward(ctx, dcol):
        x, offset = ctx.saved_tensors
        B, H, W, C = (int(v) for v in x.shape)
        dcol = dcol.contiguous()
        dx = torch.empty_like(x)
        doff = torch.zeros_like(offset)
        lib = _lib.load()
        if hip_ops.deterministic():
            # gather form of d x (no float atomics): bitwise repeatable
            nws = lib.sgv3d_deform_im2col3x3_backward_det_workspace_bytes(B, H, W)
            if nws == 0:
                raise _lib.SGV3DError(f"deform_im2col3x3_backward_det: shape {B}x{H}x{W} out of range")
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
            with torch.cuda.device(x.device), prof("deform_im2col3x3_backward_det"):
                rc = lib.sgv3d_deform_im2col3x3_backward_det(B, H, W, C, int(ctx.groups), x.data_ptr(), offset.data_ptr(),
                                                             int(offset.shape[-1]), dcol.data_ptr(), dx.data_ptr(), doff.data_ptr(),
                                                             int(doff.shape[-1]), ws.data_ptr(), nws, _st(x))
            _lib.check(rc, "sgv3d_deform_im2col3x3_backward_det")
            return dx, doff, None
        with torch.cuda.device(x.device), prof("deform_im2col3x3_backward"):
            rc = lib.sgv3d_deform_im2col3x3_backward(B, H, W, C, int(ctx.groups), x.data_ptr(), offset.data_ptr(),
                                                     int(offset.shape[-1]), dcol.data_ptr(), dx.data_ptr(),
                                                     doff.data_ptr(), int(doff.shape[-1]), _st(x))
        _lib.check(rc, "sgv3d_deform_im2col3x3_backward")
        return dx, doff, None


def deform_im2col3x3(x, offset, groups):
    """Deformable bilinear im2col of a 3x3 / pad 1 DCNv1: x NHWC [B,H,W,C], offset NHWC [B,H,W,>=18] ->
    col [B,H,W,groups*9*(C/groups)], differentiable in x and offset."""
    return _DeformIm2col.apply(x.contiguous(), offset.contiguous(), groups)


def deform_conv3x3_covers(channels, groups, out_channels):
    """The shapes ``deform_conv3x3`` takes -- those of sgv3d_deform_conv3x3_forward_bf16 and
    sgv3d_deform_conv3x3_backward_weight_bf16: at most 8 groups, channels per group a multiple of 32, outputs per group a
    multiple of 4."""
    return hip_ops.deform_conv3x3_bf16_covers(channels, groups, out_channels)


def deform_conv3x3_backward_weight(x, offset, dy, groups, split=0, out=None):
    """dW (OIHW [cout, C / groups, 3, 3]) of the deformable 3x3 convolution with the samples recomputed from ``x`` and ``offset``
    (sgv3d_deform_conv3x3_backward_weight_bf16: bf16 operands, f32 accumulation, fixed-order sums).  NHWC f32 ``x`` [B, H, W, C],
    ``offset`` [B, H, W, >= 18], ``dy`` [B, H, W, cout]; ``split``: pixel ranges (0 = the library's rule); ``out``: a contiguous
    f32 tensor of dW's shape to write (a gradient slot)."""
    B, H, W, C = (int(v) for v in x.shape)
    cout, g = int(dy.shape[-1]), int(groups)
    assert x.is_contiguous() and offset.is_contiguous() and dy.is_contiguous() and x.dtype == offset.dtype == dy.dtype == torch.float32
    assert tuple(dy.shape[:3]) == (B, H, W) and tuple(offset.shape[:3]) == (B, H, W) and cout % g == 0
    lib = _lib.load()
    nws = int(lib.sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes(B, H, W, C, g, cout // g, int(split)))
    if nws == 0:
        raise _lib.SGV3DError(f"deform_conv3x3_backward_weight: shape not covered (channels={C} groups={g} outputs={cout})")
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    shape = (cout, C // g, 3, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == shape and out.is_contiguous() and out.dtype == torch.float32 and out.device == x.device
    P = B * H * W
    with torch.cuda.device(x.device), prof("dcn_wgrad_bf16", 2.0 * P * cout * 9 * (C // g), 4.0 * (P * (C + 18 + cout) + cout * 9 * (C // g))):
        rc = lib.sgv3d_deform_conv3x3_backward_weight_bf16(B, H, W, C, g, cout // g, x.data_ptr(), offset.data_ptr(), int(offset.shape[-1]),
                                                           dy.data_ptr(), out.data_ptr(), int(split), ws.data_ptr(), nws, _st(x))
    _lib.check(rc, "sgv3d_deform_conv3x3_backward_weight_bf16")
    return out


class _DeformConv(torch.autograd.Function):
    """The deformable 3x3 convolution as ONE differentiable operator: saves x, offset and weight -- nothing of the column size."""

    @staticmethod
    def forward(ctx, x, offset, weight, groups):
        packed = hip_ops.PackedDeformBf16(weight, groups)                  # one launch: the current weights, rounded once
        y = hip_ops.deform_conv3x3_bf16(x, offset, packed, out_dtype=torch.float32)
        ctx.save_for_backward(x, offset, weight)
        ctx.groups = int(groups)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, offset, weight = ctx.saved_tensors
        g = ctx.groups
        B, H, W, C = (int(v) for v in x.shape)
        cout, cpg = int(weight.shape[0]), int(weight.shape[1])
        opg = cout // g
        dy = dy.contiguous()
        dx = doff = dw = None
        if ctx.needs_input_grad[2]:
            dw = deform_conv3x3_backward_weight(x, offset, dy, g, out=grad_slots.claim(weight))
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            from . import conv_grad
            # the column gradient, transient: one 1x1 data gradient per group (k = tap * cpg + ci) into one buffer ...
            dcol = torch.empty(B, H, W, 9 * C, dtype=torch.float32, device=x.device)
            w = weight.detach()
            for gi in range(g):
                wg = w[gi * opg:(gi + 1) * opg].permute(0, 2, 3, 1).reshape(opg, 9 * cpg, 1, 1)
                dyg = dy if g == 1 else dy[..., gi * opg:(gi + 1) * opg].contiguous()
                dg = conv_grad.conv2d_backward_data(dyg, wg, (H, W))
                dcol[..., gi * 9 * cpg:(gi + 1) * 9 * cpg].copy_(dg[..., :9 * cpg])
                del dg, dyg
            # ... consumed by the gather-form sampling adjoint in every mode: no float atomics, bitwise repeatable
            dx = torch.empty_like(x)
            doff = torch.zeros_like(offset)
            lib = _lib.load()
            nws = lib.sgv3d_deform_im2col3x3_backward_det_workspace_bytes(B, H, W)
            if nws == 0:
                raise _lib.SGV3DError(f"deform_im2col3x3_backward_det: shape {B}x{H}x{W} out of range")
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
            with torch.cuda.device(x.device), prof("deform_im2col3x3_backward_det"):
                rc = lib.sgv3d_deform_im2col3x3_backward_det(B, H, W, C, g, x.data_ptr(), offset.data_ptr(), int(offset.shape[-1]),
                                                             dcol.data_ptr(), dx.data_ptr(), doff.data_ptr(), int(doff.shape[-1]),
                                                             ws.data_ptr(), nws, _st(x))
            _lib.check(rc, "sgv3d_deform_im2col3x3_backward_det")
            del dcol
            if not ctx.needs_input_grad[0]:
                dx = None
            if not ctx.needs_input_grad[1]:
                doff = None
        return dx, doff, dw, None


def deform_conv3x3(x, offset, weight, groups):
    """mmcv DeformConv2d (DCNv1: 3x3, stride 1, pad 1, dilation 1, deform_groups 1, no bias) of the mixed-precision training step
    (bf16 operands, f32 tensors and accumulation), differentiable in ``x``, ``offset`` and ``weight``: x NHWC f32 [B, H, W, C],
    offset NHWC f32 [B, H, W, >= 18], weight OIHW [cout, C / groups, 3, 3] -> NHWC f32 [B, H, W, cout].  A shape
    ``deform_conv3x3_covers`` refuses is an error."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and offset.dtype == torch.float32 and weight.dtype == torch.float32):
        raise _lib.SGV3DError("deform_conv3x3: NHWC float32 tensors on the GPU")
    C, cout = int(x.shape[-1]), int(weight.shape[0])
    if (tuple(weight.shape[2:]) != (3, 3) or int(weight.shape[1]) * int(groups) != C or int(offset.shape[-1]) < 18
            or not deform_conv3x3_covers(C, groups, cout)):
        raise _lib.SGV3DError(f"deform_conv3x3: shape not covered (channels={C} groups={int(groups)} weight={tuple(weight.shape)} "
                              f"offset channels={int(offset.shape[-1])})")
    return _DeformConv.apply(x.contiguous(), offset.contiguous(), weight.contiguous(), int(groups))
