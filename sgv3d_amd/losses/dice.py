"""``DiceLoss`` of losses/dice.py:12-130 on the MI355X (csrc/dice_loss.hip): the forward is two launches (per-class partial
sums over a fixed grid, a one-workgroup finish), the backward one launch that recomputes the activation; the sums are
float64 and added in a fixed order, so a value and a gradient are bitwise repeatable, and nothing waits on the host, so
forward + backward capture into the training step's hipGraph.

Constructor and ``forward(y_pred, y_true)`` keep the reference's meaning:

* activation: ``from_logits=True`` is softmax over the classes in ``mode='multiclass'`` and a sigmoid per element in the
  other modes; ``from_logits=False`` takes ``y_pred`` as probabilities;
* ``multiclass``: ``y_true`` class ids ``[N, *spatial]``, ``t[b, c, p] = (y_true[b, p] == c)``, a pixel whose id is
  ``ignore_index`` is masked (``m = 0``) in ``p`` and ``t``; ``binary``: both tensors as ``[N, 1, -1]``; ``multilabel``:
  ``[N, C, -1]`` with hard or soft targets of any float or integer dtype; in both, an element whose target equals
  ``ignore_index`` is masked;
* per class over batch and pixels: ``I = sum p t``, ``P = sum p``, ``T = sum t``,
  ``score = (2 I + smooth) / max(P + T + smooth, eps)``; ``loss_c = 1 - score`` or, with ``log_loss``,
  ``-log(max(score, eps))``; a class with ``T == 0`` counts nothing; ``classes`` selects (with multiplicity) the classes
  whose mean is the result.

Where this differs from the reference:

1. CPU tensors raise: there is no CPU path (as for ``FocalLoss``).
2. ``uint8`` labels (what ``downsample_gt_semantic`` returns; the reference's ``F.one_hot`` refuses them) are accepted and
   ``int64`` labels are read in place, neither is converted; ``ignore_index`` is honoured for both.
3. A ``multiclass`` label outside ``[0, C)`` that is not the ignore index matches no class (the reference raises inside
   ``F.one_hot``; a check on the device would need a host wait).
4. ``mode='multiclass'`` covers ``2 <= C <= 32`` (a thread keeps one pixel's classes in registers; SGV3D has 7):
   ``hip_ops.dice_covers(mode, C)``; anything else raises before any launch.  ``binary`` and ``multilabel`` take any ``C``.

``y_pred`` must be float32.  ``multiclass`` with ``from_logits=False`` has no softmax to fuse the one-hot into: its targets
are expanded to a float ``[N, C, P]`` tensor by torch before the same kernels run (not a path of the shipped configs).
"""
import torch
from torch.nn.modules.loss import _Loss

from .. import _lib, hip_ops
from ..hip_ops import prof
from .focal import BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE

__all__ = ['DiceLoss']

ACT_NONE, ACT_SIGMOID, ACT_SOFTMAX = 0, 1, 2


class _Dice(torch.autograd.Function):
    """``cfg`` = (layout, target_kind, activation, ignore_index or None, smooth, eps, log_loss)."""

    @staticmethod
    def forward(ctx, pred, target, weight, cfg):
        (batch, classes, pixels, sb, sc, sp), kind, act, ignore_index, smooth, eps, log_loss = cfg
        lib = _lib.load()
        dev = pred.device
        nws = lib.sgv3d_dice_loss_workspace_bytes(classes)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        saved = torch.empty(classes, 4, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev), prof("dice_loss"):
            rc = lib.sgv3d_dice_loss_forward(
                batch, classes, pixels, pred.data_ptr(), sb, sc, sp, target.data_ptr(), kind, act,
                0 if ignore_index is None else int(ignore_index), 0 if ignore_index is None else 1, float(smooth), float(eps),
                1 if log_loss else 0, weight.data_ptr(), out.data_ptr(), saved.data_ptr(), ws.data_ptr(), nws,
                _lib.stream_handle(dev))
        _lib.check(rc, "sgv3d_dice_loss_forward")
        ctx.cfg = cfg
        ctx.save_for_backward(pred, target, saved)      # the four numbers per class, not a gradient tensor
        return out[0]

    @staticmethod
    def backward(ctx, g):
        pred, target, saved = ctx.saved_tensors
        (batch, classes, pixels, sb, sc, sp), kind, act, ignore_index, smooth, eps, _ = ctx.cfg
        dev = pred.device
        up = g.to(torch.float32).contiguous()           # stays on the device: the kernel reads the upstream scalar itself
        grad = torch.empty_strided(pred.size(), pred.stride(), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), prof("dice_loss_backward"):
            rc = _lib.load().sgv3d_dice_loss_backward(
                batch, classes, pixels, pred.data_ptr(), sb, sc, sp, target.data_ptr(), kind, act,
                0 if ignore_index is None else int(ignore_index), 0 if ignore_index is None else 1, float(smooth), float(eps),
                saved.data_ptr(), up.data_ptr(), grad.data_ptr(), _lib.stream_handle(dev))
        _lib.check(rc, "sgv3d_dice_loss_backward")
        return grad, None, None, None


class DiceLoss(_Loss):
    def __init__(self, mode, classes=None, log_loss=False, from_logits=True, smooth=0.0, ignore_index=None, eps=1e-7):
        assert mode in {BINARY_MODE, MULTILABEL_MODE, MULTICLASS_MODE}
        super().__init__()
        self.mode = mode
        if classes is not None:
            assert mode != BINARY_MODE, "Masking classes is not supported with mode=binary"
            classes = [int(c) for c in (classes.tolist() if torch.is_tensor(classes) else classes)]
        self.classes = classes
        self.from_logits = from_logits
        self.smooth = smooth
        self.eps = eps
        self.log_loss = log_loss
        self.ignore_index = ignore_index
        self._weights = {}

    def _class_weight(self, C, device):
        """f32 ``[C]`` on ``device``: the multiplicity of each class in ``classes`` / ``len(classes)`` (1/C without a list).
        Built once per (device, C), outside any graph capture."""
        key = (str(device), C)
        w = self._weights.get(key)
        if w is None:
            if self.classes is None:
                host = torch.full((C,), 1.0 / C, dtype=torch.float64)
            else:
                host = torch.zeros(C, dtype=torch.float64)
                for c in self.classes:
                    if not -C <= c < C:
                        raise IndexError(f"DiceLoss: class {c} of `classes` is out of range for {C} channels")
                    host[c] += 1.0 / len(self.classes)
            w = self._weights[key] = host.to(torch.float32).to(device)
        return w

    def forward(self, y_pred, y_true):
        if not y_pred.is_cuda:
            raise RuntimeError("sgv3d_amd.losses runs on the MI355X only (no CPU fallback)")
        if y_pred.dtype != torch.float32:
            raise TypeError(f"DiceLoss: y_pred must be float32, got {y_pred.dtype}")
        assert y_true.size(0) == y_pred.size(0)
        assert y_pred.dim() >= 2, "y_pred must be [N, C, *spatial]"
        y_true = y_true.to(y_pred.device)
        N, C = int(y_pred.shape[0]), int(y_pred.shape[1])
        if not hip_ops.dice_covers(self.mode, C):
            raise _lib.SGV3DError(f"DiceLoss: mode {self.mode!r} with {C} classes is not covered (hip_ops.dice_covers)")
        ignore_index = self.ignore_index

        if self.mode == MULTICLASS_MODE and self.from_logits:
            P = y_pred[0, 0].numel()
            assert tuple(y_true.shape) == (N,) + tuple(y_pred.shape[2:]), "y_true must be [N, *spatial] class ids"
            x = y_pred
            st = x.stride()
            if not all(st[i] == st[i + 1] * x.shape[i + 1] for i in range(2, x.dim() - 1)):
                x = x.contiguous()                  # the spatial dims must be one run of pixels; batch / class strides are free
                st = x.stride()
            sp = st[-1] if x.dim() > 2 else 1
            if y_true.dtype == torch.uint8:
                kind, tgt = 0, y_true.contiguous()
            else:
                kind, tgt = 1, y_true.long().contiguous()
            layout, act = (N, C, P, st[0], st[1], sp), ACT_SOFTMAX
        else:
            act = ACT_SIGMOID if self.from_logits else ACT_NONE
            kind = 2
            if self.mode == MULTICLASS_MODE:
                # probabilities against class ids: the one-hot targets as floats, -1 standing for a masked pixel
                assert tuple(y_true.shape) == (N,) + tuple(y_pred.shape[2:]), "y_true must be [N, *spatial] class ids"
                ids = y_true.reshape(N, 1, -1).long()
                tgt = (ids == torch.arange(C, device=ids.device).view(1, C, 1)).to(torch.float32)
                if ignore_index is not None:
                    tgt = torch.where(ids == int(ignore_index), tgt.new_tensor(-1.0), tgt)
                    ignore_index = -1
                x = y_pred.reshape(N, C, -1)
            elif self.mode == BINARY_MODE:
                assert y_true.numel() == y_pred.numel(), "binary mode: y_pred and y_true must have the same number of elements"
                x, tgt, C = y_pred.reshape(N, 1, -1), y_true.reshape(N, 1, -1), 1
            else:
                x, tgt = y_pred.reshape(N, C, -1), y_true.reshape(N, C, -1)
                assert x.shape == tgt.shape, "multilabel mode: y_true must be [N, C, *spatial]"
            x = x.contiguous()
            tgt = tgt.to(torch.float32).contiguous()
            P = int(x.shape[2])
            layout = (N, C, P, C * P, P, 1)
        if N * P == 0:
            raise ValueError("DiceLoss: empty input")
        cfg = (layout, kind, act, ignore_index, self.smooth, self.eps, self.log_loss)
        return _Dice.apply(x, tgt, self._class_weight(C, x.device), cfg)
