"""Float64 restatements for the bf16-activation-storage tests (test_bf16_storage_cpu.py checks them against torch's float64 autograd;
test_bf16_storage_gpu.py holds the kernels against them).  Everything here runs on the CPU."""
import torch
import torch.nn.functional as F


def bn_act(x, res, gamma, beta, eps, relu, dy):
    """Training-mode BatchNorm (+ residual) (+ ReLU) over [pixels, C] float64 and its backward, written out:
    returns dict(mean, var, invstd, scale, shift, pre, y, dz, dbeta, dgamma, xhat, dx, dres)."""
    P = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)                      # biased
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mean) if gamma is None else gamma
    b = torch.zeros_like(mean) if beta is None else beta
    scale = g * invstd
    shift = b - mean * scale
    pre = x * scale + shift
    if res is not None:
        pre = pre + res
    y = pre.clamp_min(0) if relu else pre
    dz = dy * (pre > 0) if relu else dy
    dbeta = dz.sum(0)
    xhat = (x - mean) * invstd
    dgamma = (dz * xhat).sum(0)
    dx = scale * (dz - dbeta / P - xhat * dgamma / P)
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, pre=pre, y=y, dz=dz, dbeta=dbeta, dgamma=dgamma, xhat=xhat,
                dx=dx, dres=dz)


def running(stat_old, mean, var, pixels, momentum):
    """(running_mean, running_var) after one training-mode call (unbiased variance, like nn.BatchNorm2d)."""
    unbiased = var * pixels / (pixels - 1) if pixels > 1 else var
    return (1 - momentum) * stat_old[0] + momentum * mean, (1 - momentum) * stat_old[1] + momentum * unbiased


def wgrad_einsum(x, dy, k, stride, pad, dil):
    """dW [cout, cin, k, k] of y = conv2d(x, W) for NHWC float64 ``x`` [B, H, W, cin], ``dy`` [B, OH, OW, cout]: an einsum over the
    unfolded input."""
    B, H, W, cin = x.shape
    cout = dy.shape[-1]
    cols = F.unfold(x.permute(0, 3, 1, 2), k, dilation=dil, padding=pad, stride=stride)          # [B, cin * k * k, L]
    d = dy.reshape(B, -1, cout)                                                                   # [B, L, cout]
    return torch.einsum('blo,bkl->ok', d, cols).reshape(cout, cin, k, k)


def _bn_train(m, x):
    return F.batch_norm(x, None, None, m.weight.double(), m.bias.double(), True, 0.0, m.eps)


def _conv(m, x):
    return F.conv2d(x, m.weight.double(), None, m.stride, m.padding, m.dilation)


def resnet_stages(r, x):
    """The stages of a blocks.ResNet (BasicBlock or Bottleneck, BatchNorm with batch statistics) in float64 on an NCHW map ``x`` that
    enters stage 1; the parameters are read from ``r`` (a CPU copy of the module: its float32 leaves receive the gradients through the
    differentiable ``.double()``).  Returns the maps of ``r.out_indices``."""
    outs = []
    for i, name in enumerate(r.res_layers):
        for b in getattr(r, name):
            idn = x if b.downsample is None else _bn_train(b.downsample[1], _conv(b.downsample[0], x))
            out = F.relu(_bn_train(b.bn1, _conv(b.conv1, x)))
            if hasattr(b, 'conv3'):
                out = F.relu(_bn_train(b.bn2, _conv(b.conv2, out)))
                x = F.relu(_bn_train(b.bn3, _conv(b.conv3, out)) + idn)
            else:
                x = F.relu(_bn_train(b.bn2, _conv(b.conv2, out)) + idn)
        if i in r.out_indices:
            outs.append(x)
    return outs
