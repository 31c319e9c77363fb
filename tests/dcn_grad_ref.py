"""float64 restatement of the gradients of the deformable 3x3 convolution (DCNv1: 3x3, stride 1, pad 1, deform_groups 1, no
bias) from the oracle's ``deform_im2col3x3`` / ``deform_conv3x3``: dW as the explicit pixel sum the kernel of csrc/dcn_grad.hip
forms, dx and d offset through float64 autograd.  Tensors in the kernels' layouts (NHWC, column tensor [B, H, W, groups * 9 * cpg]
with k = tap * cpg + ci, weights OIHW), on whatever device the inputs live on."""
import torch

from oracle import torch_model as TM


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bf16_round(t):
    """Round to nearest-even bf16, returned as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def col_to_kernel_layout(col, groups):
    """oracle col [B, C, 9, H, W] -> [B, H, W, groups * 9 * cpg] (group, tap, channel)."""
    B, C, _, H, W = col.shape
    cpg = C // groups
    return col.reshape(B, groups, cpg, 9, H, W).permute(0, 4, 5, 1, 3, 2).reshape(B, H, W, groups * 9 * cpg).contiguous()


def column_tensor(x, offset, groups):
    """float64 column tensor in the kernel layout from NHWC ``x`` [B, H, W, C] and ``offset`` [B, H, W, >= 18]."""
    return col_to_kernel_layout(TM.deform_im2col3x3(nchw(x.to(torch.float64)), nchw(offset[..., :18].to(torch.float64))), groups)


def dw_from_col(col, dy, groups, rounded=False):
    """dW[g opg + co][ci][r][s] = sum_p dy[p][g opg + co] * col[p][g][3 r + s][ci] in float64, and the sum of the absolute
    values of the terms (the scale of an a-priori rounding bound).  ``rounded``: both operands rounded to bf16 first."""
    B, H, W, K = col.shape
    cout = dy.shape[-1]
    cpg, opg = K // (9 * groups), cout // groups
    c = (bf16_round(col) if rounded else col.to(torch.float64)).reshape(B * H * W, groups, 9, cpg)
    d = (bf16_round(dy) if rounded else dy.to(torch.float64)).reshape(B * H * W, groups, opg)
    dw = torch.einsum('pgo,pgtc->goct', d, c).reshape(cout, cpg, 3, 3)
    mag = torch.einsum('pgo,pgtc->goct', d.abs(), c.abs()).reshape(cout, cpg, 3, 3)
    return dw, mag


def backward(x, offset, weight, dy, groups, rounded=False):
    """{'dw', 'dw_abs', 'dx', 'doff', 'y'}: dW by the explicit sum over the oracle's column tensor (``rounded``: column tensor and
    dy rounded to bf16 first), dx NHWC and d offset NHWC [B, H, W, 18] by float64 autograd of the oracle's deform_conv3x3."""
    xr = nchw(x.to(torch.float64)).requires_grad_(True)
    orr = nchw(offset[..., :18].to(torch.float64)).requires_grad_(True)
    wr = weight.to(torch.float64).clone().requires_grad_(True)
    y = TM.deform_conv3x3(xr, orr, wr, groups)
    y.backward(nchw(dy.to(torch.float64)))
    dw, mag = dw_from_col(column_tensor(x, offset, groups), dy, groups, rounded)
    return {'dw': dw, 'dw_abs': mag, 'dw_autograd': wr.grad, 'dx': nhwc(xr.grad), 'doff': nhwc(orr.grad), 'y': nhwc(y.detach())}
