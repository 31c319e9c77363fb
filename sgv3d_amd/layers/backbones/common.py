"""``MLPBlock`` and ``LayerNorm2d`` of the reference's layers/backbones/common.py (same constructor signatures and
state_dict names), plus the device calls the SAM encoder shares: LayerNorm over the channels of an NHWC map, the exact
GELU, and a linear layer's ``PackedConv`` kept per parameter version.

Inference only.  ``torch.nn`` leaves hold the parameters; arithmetic runs through the C ABI on NHWC float32 buffers.
"""
from typing import Type

import torch
from torch import nn

from ... import _lib
from ...hip_ops import PackedConv


def require_device(x, what, bf16_ok=False):
    """The house rule: no CPU path and no autograd path -- both raise.  ``bf16_ok``: the layer also takes the bf16 tensors of the
    encoder's bf16 mode (hip_ops.VIT_BF16)."""
    if not isinstance(x, torch.Tensor):
        raise _lib.SGV3DError(f"{what}: a tensor is expected")
    if x.requires_grad and torch.is_grad_enabled():
        raise _lib.SGV3DError(f"{what} is inference only: the input requires grad and there is no backward; "
                              "call it under torch.no_grad() or on a detached tensor")
    if not x.is_cuda:
        raise _lib.SGV3DError(f"{what}: the input must be a tensor on the GPU (there is no CPU fallback)")
    if x.dtype != torch.float32 and not (bf16_ok and x.dtype == torch.bfloat16):
        raise _lib.SGV3DError(f"{what}: float32 input expected, got {x.dtype}")


def layernorm(x, weight, bias, eps, out=None, out_dtype=None):
    """LayerNorm over the last dimension of a contiguous f32 tensor (``nn.LayerNorm(C)``; on NHWC maps also ``LayerNorm2d``).
    ``out_dtype=torch.bfloat16`` (or a bf16 ``out``): the same f32 result rounded once to bf16 (sgv3d_layernorm_bf16out)."""
    assert x.is_contiguous() and x.dtype == torch.float32
    c = int(x.shape[-1])
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or torch.float32, device=x.device)
    assert out.is_contiguous() and out.shape == x.shape and out.dtype in (torch.float32, torch.bfloat16)
    assert out_dtype is None or out.dtype == out_dtype
    lib = _lib.load()
    bf16 = out.dtype == torch.bfloat16
    fn, name = (lib.sgv3d_layernorm_bf16out, "sgv3d_layernorm_bf16out") if bf16 else (lib.sgv3d_layernorm, "sgv3d_layernorm")
    with torch.cuda.device(x.device):
        rc = fn(x.numel() // c, c, x.data_ptr(), weight.data_ptr(), bias.data_ptr(), float(eps), out.data_ptr(),
                _lib.stream_handle(x.device))
    _lib.check(rc, name)
    return out


def gelu_(x):
    """Exact (erf) GELU in place; on a bf16 tensor the f32 formula on the widened value, rounded once (sgv3d_gelu_bf16)."""
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
    lib = _lib.load()
    bf16 = x.dtype == torch.bfloat16
    fn, name = (lib.sgv3d_gelu_bf16, "sgv3d_gelu_bf16") if bf16 else (lib.sgv3d_gelu, "sgv3d_gelu")
    with torch.cuda.device(x.device):
        rc = fn(x.numel(), x.data_ptr(), x.data_ptr(), _lib.stream_handle(x.device))
    _lib.check(rc, name)
    return x


class PackedParam:
    """The ``PackedConv`` of one linear layer or convolution, made again when its parameters change: the key is the
    storage address and version counter of weight and bias, which ``load_state_dict``, an optimiser step and ``.to()`` all move."""

    def __init__(self):
        self._key = None
        self._pc = None

    def get(self, weight, bias=None, **kw):
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in (weight, bias) if t is not None)
        if key != self._key:
            w = weight.detach()
            if w.dim() == 2:        # nn.Linear on [B, H, W, C] tokens is a 1x1 convolution of the NHWC map
                w = w.reshape(w.shape[0], w.shape[1], 1, 1)
            self._pc = PackedConv(w, shift=None if bias is None else bias.detach(), **kw)
            self._key = key
        return self._pc


class MLPBlock(nn.Module):
    def __init__(self, embedding_dim: int, mlp_dim: int, act: Type[nn.Module] = nn.GELU) -> None:
        super().__init__()
        self.lin1 = nn.Linear(embedding_dim, mlp_dim)
        self.lin2 = nn.Linear(mlp_dim, embedding_dim)
        self.act = act()
        if not isinstance(self.act, nn.GELU) or getattr(self.act, 'approximate', 'none') != 'none':
            raise NotImplementedError("MLPBlock: only the exact nn.GELU has a kernel")
        self._p1, self._p2 = PackedParam(), PackedParam()

    def forward(self, x: torch.Tensor, residual=None) -> torch.Tensor:
        """x [B, H, W, C] on the device -> lin2(gelu(lin1(x))) (+ ``residual``, added in lin2's epilogue).  A bf16 ``x`` (the
        encoder's bf16 mode): the hidden map stays bf16, lin2 writes f32."""
        require_device(x, "MLPBlock", bf16_ok=True)
        with torch.no_grad():
            h = self._p1.get(self.lin1.weight, self.lin1.bias)(x, out_dtype=x.dtype)
            gelu_(h)
            return self._p2.get(self.lin2.weight, self.lin2.bias)(h, residual=residual)


class LayerNorm2d(nn.Module):
    def __init__(self, num_channels: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.eps = eps

    def forward_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        return layernorm(x, self.weight, self.bias, self.eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, C, H, W] as in the reference; a permuted view of the NHWC result comes back."""
        require_device(x, "LayerNorm2d")
        with torch.no_grad():
            return self.forward_nhwc(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
