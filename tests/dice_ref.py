"""The dice loss of the reference's ``losses`` package restated with torch operators in whatever dtype the inputs have
(float64 in the tests; float32 on the GPU as the baseline of tools/dice_loss_bench.py).  Written from the semantics, not from
the reference's text; tests/test_dice_loss_cpu.py pins it to the reference's own values and autograd gradients
(tests/golden/dice_loss.npz) to 1e-12.  Differentiable through autograd: torch's ``clamp_min`` passes the gradient where the
value is >= the bound, and a class without a true element is multiplied by 0."""
import torch


def dice_loss(y_pred, y_true, mode, classes=None, log_loss=False, from_logits=True, smooth=0.0, ignore_index=None, eps=1e-7):
    """``y_pred`` [N, C, *spatial] (binary: any shape with N first); ``y_true`` class ids [N, *spatial] (multiclass, any integer
    dtype; an id outside [0, C) that is not ``ignore_index`` matches no class) or same-size targets (binary / multilabel)."""
    assert mode in ("binary", "multiclass", "multilabel")
    n = y_pred.shape[0]
    if from_logits:
        p = torch.softmax(y_pred, dim=1) if mode == "multiclass" else torch.sigmoid(y_pred)
    else:
        p = y_pred
    if mode == "multiclass":
        c = y_pred.shape[1]
        p = p.reshape(n, c, -1)
        ids = y_true.reshape(n, 1, -1).long()
        t = (ids == torch.arange(c, device=ids.device).view(1, c, 1)).to(p.dtype)
        m = torch.ones_like(ids, dtype=p.dtype) if ignore_index is None else (ids != ignore_index).to(p.dtype)
    else:
        c = 1 if mode == "binary" else y_pred.shape[1]
        p = p.reshape(n, c, -1)
        raw = y_true.reshape(n, c, -1)
        m = torch.ones_like(p) if ignore_index is None else (raw != ignore_index).to(p.dtype)
        t = raw.to(p.dtype)
    p, t = p * m, t * m
    inter = (p * t).sum(dim=(0, 2))
    psum = p.sum(dim=(0, 2))
    tsum = t.sum(dim=(0, 2))
    score = (2.0 * inter + smooth) / (psum + tsum + smooth).clamp_min(eps)
    loss = -torch.log(score.clamp_min(eps)) if log_loss else 1.0 - score
    loss = loss * (tsum > 0).to(loss.dtype)
    if classes is not None:
        loss = loss[torch.as_tensor(list(classes), dtype=torch.long, device=loss.device)]
    return loss.mean()


def loss_bar(ref64, ref32):
    """|device - ref64| allowed for a loss: four times the reference's own float32 error, floored at two float32 ulps of the
    result (the float32 run is sometimes exact by luck)."""
    return max(4.0 * abs(float(ref32) - float(ref64)), 2.0 ** -22 * max(1.0, abs(float(ref64))))


def grad_bar(ref64, ref32):
    """Largest absolute gradient error allowed: four times the reference's float32 error, floored at 2^-21 of the largest
    gradient."""
    import numpy as np
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    return max(4.0 * float(np.abs(ref32 - ref64).max()), 2.0 ** -21 * float(np.abs(ref64).max()))
