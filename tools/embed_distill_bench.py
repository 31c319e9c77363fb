#!/usr/bin/env python3
"""Forward + backward of ``losses.EmbedDistillation`` on the assist map of cfg-2 (256 channels, 54 x 96, the NCHW view of an
NHWC buffer) at batch 2 and 8 with half the frames warped, against the same operation written with torch operators in float32
on the same GPU (tests/embed_distill_ref.py: the warp materialised, then the loss through autograd); and the materialising
warp (``distill.warp_embed``) alone against the restatement's.  One process, HIP events, median of 10 after 3 warm-up calls, the
two paths alternating.  Writes profiles/embed_distill_bench.json and prints it as one JSON line.

    python tools/embed_distill_bench.py [--out profiles/embed_distill_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import embed_distill_ref as ER  # noqa: E402
from sgv3d_amd import distill, hip_ops  # noqa: E402
from sgv3d_amd.losses import EmbedDistillation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_distill_bench.json"))
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
C, H, W = 256, 54, 96
WEIGHT = 1000.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3            # microseconds


def matrices(rng, batch):
    """inv(M) of rectifications of the size the reference draws (ratio ~ N(1, 0.2), roll ~ N(0, 2 deg)) on the 54 x 96 grid."""
    out = np.tile(np.eye(3), (batch, 1, 1))
    for b in range(0, batch, 2):                 # every other frame is warped
        zoom, a = rng.uniform(0.85, 1.25), np.deg2rad(rng.uniform(-3, 3))
        cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
        lin = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) / zoom
        out[b, :2, :2] = lin
        out[b, :2, 2] = np.array([cx, cy]) - lin @ np.array([cx, cy]) + rng.uniform(-1, 1, 2)
    return out, np.array([1 - b % 2 for b in range(batch)], np.uint8)


rows = []
for batch in (2, 8):
    rng = np.random.default_rng(batch)
    g = torch.Generator().manual_seed(batch)
    store = torch.randn(batch, H, W, C, generator=g).to(dev)          # the NHWC buffer train_forward hands out a view of
    teacher = torch.randn(batch, H, W, C, generator=g).to(dev)
    minv_h, warped_h = matrices(rng, batch)
    minv, warped = torch.from_numpy(minv_h).to(dev), torch.from_numpy(warped_h).to(dev)
    loss_fn = EmbedDistillation(WEIGHT)

    def device_path():
        x = store.permute(0, 3, 1, 2).detach().requires_grad_(True)
        loss_fn(x, teacher, minv, warped).backward()
        return x.grad

    def torch_path():
        x = store.permute(0, 3, 1, 2).detach().requires_grad_(True)
        target, dead = ER.warp_batch(teacher, minv_h, warped_h, dtype=torch.float32)
        ER.distill_loss(x, target, dead, WEIGHT).backward()
        return x.grad

    def device_warp():
        return distill.warp_embed(teacher, minv, warped)

    def torch_warp():
        return ER.warp_batch(teacher, minv_h, warped_h, dtype=torch.float32)[0]

    for _ in range(args.warmup):
        gd, gt = device_path(), torch_path()
        wd, wt = device_warp(), torch_warp()
    torch.cuda.synchronize()
    err = float((gd - gt).abs().max() / gt.abs().max())
    werr = float((wd - wt).abs().max())
    t = {k: [] for k in ("dev", "ref", "wdev", "wref")}
    for _ in range(args.repeats):               # alternating, so that clocks and caches are shared evenly
        t["dev"].append(timed(device_path))
        t["ref"].append(timed(torch_path))
        t["wdev"].append(timed(device_warp))
        t["wref"].append(timed(torch_warp))
    hip_ops.PROFILE = []                        # the forward call (two launches), the backward launch and the warp by themselves
    for _ in range(args.repeats):
        device_path()
        device_warp()
    torch.cuda.synchronize()
    per = {}
    for name, _, e0, e1, *_ in hip_ops.PROFILE:
        per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    hip_ops.PROFILE = None
    n = batch * H * W * C * 4                   # bytes of one tensor
    med = {k: statistics.median(v) for k, v in t.items()}
    fwd, bwd, wrp = (statistics.median(per[k]) for k in ("embed_distill", "embed_distill_backward", "embed_warp"))
    # unique bytes: the forward reads student and teacher once; the backward reads both and writes the gradient; the warp
    # reads the teacher and writes the output (a warped pixel's four neighbours are shared with the pixels next to it)
    rows.append({
        "shape": [batch, C, H, W], "layout": "NCHW view of an NHWC buffer", "frames_warped": int(warped_h.sum()),
        "dead_share_of_warped_frames": float(ER.warp_batch(teacher[:1], minv_h[:1], warped_h[:1])[1].float().mean()),
        "device_us_median": med["dev"], "torch_f32_us_median": med["ref"],
        "device_us_all": [round(v, 1) for v in t["dev"]], "torch_f32_us_all": [round(v, 1) for v in t["ref"]],
        "torch_over_device": med["ref"] / med["dev"], "device_not_slower": med["dev"] <= med["ref"],
        "warp_device_us_median": med["wdev"], "warp_torch_f32_us_median": med["wref"],
        "warp_device_not_slower": med["wdev"] <= med["wref"],
        "forward_two_launches_us_median": fwd, "backward_one_launch_us_median": bwd, "warp_one_launch_us_median": wrp,
        "unique_bytes": {"forward": 2 * n, "backward": 3 * n, "warp": 2 * n},
        "achieved_tb_per_s": {"forward": 2 * n / fwd / 1e6, "backward": 3 * n / bwd / 1e6, "warp": 2 * n / wrp / 1e6},
        "gradient_rel_diff_between_paths": err, "warp_abs_diff_between_paths": werr,
    })
out = {"metric": "EmbedDistillation forward + backward and warp_embed, microseconds (HIP events, median of %d after %d warm-up "
                 "calls, device path and float32 torch restatement alternating in one process)" % (args.repeats, args.warmup),
       "device": torch.cuda.get_device_name(dev), "rows": rows,
       "condition_device_not_slower_at_either_size": all(r["device_not_slower"] and r["warp_device_not_slower"] for r in rows)}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
