#!/usr/bin/env python3
"""Forward + backward of ``losses.DiceLoss('multiclass')`` on the stride-8 semantic map of cfg-5 (7 classes, 108 x 192,
channel-last, uint8 labels) at batch 2 and 8, against the same loss written with torch operators in float32 on the same GPU
(tests/dice_ref.py through autograd).  One process, HIP events, median of 10 after 3 warm-up calls, the two paths
alternating.  Writes profiles/dice_loss_bench.json and prints it as one JSON line.

    python tools/dice_loss_bench.py [--out profiles/dice_loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dice_ref  # noqa: E402
from sgv3d_amd import _lib, hip_ops  # noqa: E402
from sgv3d_amd.losses import DiceLoss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dice_loss_bench.json"))
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
C, H, W = 7, 108, 192
BLOCKS = 256                                    # workgroups of the partial pass (csrc/dice_loss.hip)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3            # microseconds


rows = []
for batch in (2, 8):
    g = torch.Generator().manual_seed(batch)
    store = (torch.randn(batch, H, W, C, generator=g) * 3).to(dev)
    labels = torch.randint(0, C, (batch, H, W), generator=g, dtype=torch.uint8).to(dev)
    dice = DiceLoss('multiclass')

    def device_path():
        x = store.permute(0, 3, 1, 2).detach().requires_grad_(True)
        dice(x, labels).backward()
        return x.grad

    def torch_path():
        x = store.permute(0, 3, 1, 2).detach().requires_grad_(True)
        dice_ref.dice_loss(x, labels, 'multiclass').backward()
        return x.grad

    for _ in range(args.warmup):
        gd, gt = device_path(), torch_path()
    torch.cuda.synchronize()
    err = float((gd - gt).abs().max() / gt.abs().max())
    t_dev, t_ref = [], []
    for _ in range(args.repeats):               # alternating, so that clocks and caches are shared evenly
        t_dev.append(timed(device_path))
        t_ref.append(timed(torch_path))
    # the forward call (two launches) and the backward launch by themselves
    hip_ops.PROFILE = []
    for _ in range(args.repeats):
        device_path()
    torch.cuda.synchronize()
    per = {}
    for name, _, e0, e1, *_ in hip_ops.PROFILE:
        per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    hip_ops.PROFILE = None
    pixels = batch * H * W
    blocks = min(BLOCKS, (pixels + 255) // 256)
    rows.append({
        "shape": [batch, C, H, W], "layout": "channel-last view", "labels": "uint8",
        "device_us_median": statistics.median(t_dev), "torch_f32_us_median": statistics.median(t_ref),
        "device_us_all": [round(v, 1) for v in t_dev], "torch_f32_us_all": [round(v, 1) for v in t_ref],
        "torch_over_device": statistics.median(t_ref) / statistics.median(t_dev),
        "device_not_slower": statistics.median(t_dev) <= statistics.median(t_ref),
        "forward_two_launches_us_median": statistics.median(per["dice_loss"]),
        "backward_one_launch_us_median": statistics.median(per["dice_loss_backward"]),
        "bytes_moved": {
            "partial_sums": {"read": pixels * C * 4 + pixels, "written": blocks * C * 3 * 8},
            "finish": {"read": blocks * C * 3 * 8 + C * 4, "written": C * 4 * 8 + 4},
            "backward": {"read": pixels * C * 4 + pixels + C * 4 * 8 + 4, "written": pixels * C * 4}},
        "gradient_rel_diff_between_paths": err,
    })
out = {"metric": "DiceLoss('multiclass') forward + backward, microseconds (HIP events, median of %d after %d warm-up calls, "
                 "device path and float32 torch restatement alternating in one process)" % (args.repeats, args.warmup),
       "device": torch.cuda.get_device_name(dev), "rows": rows,
       "condition_device_not_slower_at_either_size": all(r["device_not_slower"] for r in rows)}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
