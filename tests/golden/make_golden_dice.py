#!/usr/bin/env python3
"""Golden fixture of the dice loss, produced by EXECUTING THE REFERENCE'S OWN PYTHON in the build container (needs a checkout
of the reference, which never travels to the GPU box).

* dice_loss.npz  ``losses.dice.DiceLoss`` (losses/dice.py:12-130 over losses/_functional.py:172-187; pure torch, imported
                 unmodified).  Per case: the inputs (float32-representable), the loss and the input gradient of the
                 reference evaluated in float64, and the same in float32 on the CPU -- the yardstick of the device path's
                 bars (tests/dice_ref.py: loss_bar, grad_bar).

The maker asserts that every constructor argument a case sets, put back to its default, moves the case's float64 loss by
more than 100 x the case's loss bar: a test cannot pass with the argument ignored.  Where the reference cannot evaluate the
changed case (labels of 255 without an ``ignore_index`` fail in ``F.one_hot``), tests/dice_ref.py -- pinned to the reference
to 1e-12 on every case by this script -- stands in.

Outputs are DATA ONLY (inputs and expected outputs); no reference source text is stored.

    python tests/golden/make_golden_dice.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("SGV3D_GOLDEN_OUT", HERE)      # regenerate elsewhere to compare with the committed file
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import dice_ref  # noqa: E402

DEFAULTS = dict(classes=None, log_loss=False, from_logits=True, smooth=0.0, ignore_index=None, eps=1e-7)


def _cases():
    g = torch.Generator().manual_seed(26)

    def logits(shape, scale=3.0):
        return torch.randn(shape, generator=g) * scale

    def ids(shape, c, ignore=None, share=0.2, never=None):
        y = torch.randint(0, c, (shape[0],) + shape[2:], generator=g)
        if never is not None:
            y[y == never] = (never + 1) % c
        if ignore is not None:
            y[torch.rand(y.shape, generator=g) < share] = ignore
        return y

    out = []
    s = (3, 7, 9, 12)                                   # the BSM setting: 7 classes, softmax, every default
    out.append(("bsm", dict(mode='multiclass'), logits(s), ids(s, 7)))
    s = (2, 7, 6, 10)
    out.append(("mc_log_smooth_ignore", dict(mode='multiclass', log_loss=True, smooth=1.0, ignore_index=255), logits(s),
                ids(s, 7, ignore=255)))
    out.append(("mc_classes", dict(mode='multiclass', classes=[1, 2, 6]), logits(s), ids(s, 7)))
    out.append(("mc_classes_repeat", dict(mode='multiclass', classes=[0, 3, 3, 5]), logits(s), ids(s, 7)))
    s = (2, 5, 5, 7)
    out.append(("mc_absent_class", dict(mode='multiclass'), logits(s), ids(s, 5, never=2)))
    s = (2, 4, 3, 5)
    # every pixel carries the ignored id -- a valid class, so that without ignore_index the loss is far from 0
    out.append(("mc_all_ignored", dict(mode='multiclass', ignore_index=3), logits(s), torch.full((2, 3, 5), 3)))
    s = (2, 1, 2, 3)                                    # few pixels, so that a small smooth shows
    out.append(("bin_smooth", dict(mode='binary', smooth=0.01), logits(s), torch.randint(0, 2, s, generator=g)))
    s = (2, 3, 5, 6)
    y = torch.randint(0, 2, s, generator=g)
    y[torch.rand(s, generator=g) < 0.2] = 255
    out.append(("ml_ignore", dict(mode='multilabel', ignore_index=255), logits(s), y))
    s = (2, 4, 4, 7)
    out.append(("ml_soft_log", dict(mode='multilabel', log_loss=True), logits(s), torch.rand(s, generator=g)))
    s = (2, 4, 5, 6)
    out.append(("mc_probabilities", dict(mode='multiclass', from_logits=False), torch.softmax(logits(s), dim=1), ids(s, 4)))
    s = (2, 3, 2, 3)                                    # P + T below eps: the clamp of the denominator decides
    out.append(("ml_probabilities_eps", dict(mode='multilabel', from_logits=False, eps=0.05),
                torch.rand(s, generator=g) * 1e-3, torch.rand(s, generator=g) * 1e-3))
    s = (2, 7, 5, 8)
    x = torch.where(torch.rand(s, generator=g) < 0.5, torch.tensor(300.0), torch.tensor(-300.0))
    out.append(("mc_pm300", dict(mode='multiclass'), x, ids(s, 7)))
    return out


def _run(cls, kw, x, y, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    loss = cls(**kw)(x, y)
    loss.backward()
    return loss.detach(), x.grad


def main():
    sys.path.insert(0, REF)
    from losses import DiceLoss                         # the reference's class, as its users import it
    out = {}
    for name, kw, x, y in _cases():
        x = x.float()
        l64, g64 = _run(DiceLoss, kw, x, y, torch.float64)
        l32, g32 = _run(DiceLoss, kw, x, y, torch.float32)
        assert torch.isfinite(l64) and torch.isfinite(g64).all(), name
        # the restatement the GPU tests lean on, pinned here as well as in tests/test_dice_loss_cpu.py
        xr = x.double().requires_grad_(True)
        lr = dice_ref.dice_loss(xr, y, **kw)
        lr.backward()
        assert abs(float(lr.detach()) - float(l64)) <= 1e-12 and float((xr.grad - g64).abs().max()) <= 1e-12, name
        bar = dice_ref.loss_bar(l64, l32)
        for arg, value in kw.items():
            if arg == 'mode' or value == DEFAULTS[arg]:
                continue
            changed = dict(kw, **{arg: DEFAULTS[arg]})
            try:
                other = float(DiceLoss(**changed)(x.double(), y))
            except Exception:                           # (F.one_hot on a label of 255)
                other = float(dice_ref.dice_loss(x.double(), y, **changed))
            assert abs(other - float(l64)) > 100 * bar, (name, arg, other, float(l64), bar)
        out[name + "_x"] = x.numpy()
        out[name + "_y"] = y.numpy() if y.dtype.is_floating_point else y.numpy().astype(np.int64)
        out[name + "_kw"] = np.array(repr(kw))
        out[name + "_loss"] = np.float64(l64.item())
        out[name + "_grad"] = g64.numpy()
        out[name + "_loss32"] = np.float32(l32.item())
        out[name + "_grad32"] = g32.numpy()
        print(f"{name:24s} loss {float(l64):.9f}  |l32 - l64| {abs(float(l32) - float(l64)):.1e}  max|g| {float(g64.abs().max()):.2e}  "
              f"|g32 - g64| {float((g32.double() - g64).abs().max()):.1e}")
    assert float(out["mc_all_ignored_loss"]) == 0 and not out["mc_all_ignored_grad"].any()
    path = os.path.join(OUT, "dice_loss.npz")
    np.savez_compressed(path, **out)
    print("dice_loss.npz:", os.path.getsize(path), "bytes,", sum(k.endswith("_loss") for k in out), "cases")


if __name__ == "__main__":
    main()
