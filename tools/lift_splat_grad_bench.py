#!/usr/bin/env python3
"""Operator A/B of the differentiable fused lift-splat: forward + backward of ``ops.voxel_pooling.lift_splat`` against the
materialised composition it replaces in training (torch ``mul`` -> ``voxel_pooling`` operator, the [B, D*P, C] lifted tensor
and its gradient in HBM), at the cfg-2 and cfg-5 training shapes (batch 2) with the geometry of ``synthetic.make_mats``.

Timing: HIP events in this process, the two forms alternating, after warm-up; the adjoint kernel alone from the events
``hip_ops.prof`` puts around its launch.  Also the peak allocation of each form over forward + backward.
``python tools/lift_splat_grad_bench.py [--out profiles/lift_splat_grad_bench.json] [--iters 20]``"""
import argparse, json, os, sys, types
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgv3d_amd import _lib, hip_ops, synthetic
from sgv3d_amd.layers.backbones.lss_fpn import LSSFPN
from sgv3d_amd.ops.voxel_pooling import lift_splat, voxel_pooling

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--shapes", default="cfg2,cfg5")
args = ap.parse_args()
dev = torch.device("cuda")


def geometry(conf, B):
    """int32 [B, D*P, 3] voxel indices of the config's frustum under the synthetic calibration, and the grid."""
    ds = conf['downsample_factor'] // 2 if conf.get('is_bsm') else conf['downsample_factor']      # (bsm_lss_fpn.py:343)
    bb = types.SimpleNamespace(final_dim=conf['final_dim'], downsample_factor=ds, d_bound=conf['d_bound'])
    bounds = [conf['x_bound'], conf['y_bound'], conf['z_bound']]
    bb.frustum = LSSFPN.create_frustum(bb).to(dev)
    bb._voxel_coord_host = [float(torch.tensor(r[0] + r[2] / 2.0, dtype=torch.float32)) for r in bounds]
    bb._voxel_size_host = [float(torch.tensor(r[2], dtype=torch.float32)) for r in bounds]
    mats = synthetic.make_mats(B, device=dev, scale=conf['final_dim'][0] / 864)
    geom = LSSFPN.get_geometry_voxel_index(bb, mats['sensor2ego_mats'][:, 0], mats['sensor2virtual_mats'][:, 0], mats['intrin_mats'][:, 0],
                                           mats['ida_mats'][:, 0], mats['reference_heights'][:, 0], mats.get('bda_mat', None))
    D, fH, fW = (int(v) for v in bb.frustum.shape[:3])
    voxel_num = tuple(int(round((r[1] - r[0]) / r[2])) for r in bounds)
    return geom.reshape(B, D * fH * fW, 3).contiguous(), D, fH * fW, voxel_num


def bench(name, conf, C):
    B = args.batch
    geom, D, P, (X, Y, Z) = geometry(conf, B)
    g = torch.Generator(device=dev).manual_seed(0)
    prob0 = torch.randn(B, D, P, device=dev, generator=g).softmax(1)
    ctx0 = torch.randn(B, P, C, device=dev, generator=g)
    G = torch.randn(B, Y, X, C, device=dev, generator=g).permute(0, 3, 1, 2)      # NHWC-backed, as the BEV trunk hands it back
    kept = int(((geom[..., 0] >= 0) & (geom[..., 0] < X) & (geom[..., 1] >= 0) & (geom[..., 1] < Y) & (geom[..., 2] >= 0) & (geom[..., 2] < Z)).sum())

    def fused(prob, ctx):
        return lift_splat(geom, prob, ctx, (X, Y, Z))

    def materialised(prob, ctx):
        lifted = prob[..., None] * ctx[:, None]
        return voxel_pooling(geom, lifted.reshape(B, D * P, C).contiguous(), (X, Y, Z))

    def once(fn, ev=None):
        prob, ctx = prob0.detach().requires_grad_(True), ctx0.detach().requires_grad_(True)
        if ev:
            ev[0].record()
        fn(prob, ctx).backward(G)
        if ev:
            ev[1].record()
        return prob.grad, ctx.grad

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        once(fn)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - start

    peaks = {"fused": peak(fused), "materialised": peak(materialised)}
    gf, gm = once(fused), once(materialised)
    diff = [float((a - b).norm() / b.norm()) for a, b in zip(gf, gm)]
    for _ in range(args.warmup):
        once(fused), once(materialised)
    times = {"fused": [], "materialised": []}
    for _ in range(args.iters):                     # alternating: both forms see the same clocks and cache state
        for key, fn in (("fused", fused), ("materialised", materialised)):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            once(fn, ev)
            torch.cuda.synchronize()
            times[key].append(ev[0].elapsed_time(ev[1]))
    # the kernels of the fused form alone (events around each launch)
    hip_ops.PROFILE = []
    for _ in range(args.iters):
        once(fused)
    torch.cuda.synchronize()
    fam = {}
    for rec in hip_ops.PROFILE:
        fam.setdefault(rec[0].split('|')[0], []).append(rec[2].elapsed_time(rec[3]))
    hip_ops.PROFILE = None
    med = lambda v: sorted(v)[len(v) // 2]
    k_us = 1e3 * med(fam["lift_splat_backward"])
    unique = 4 * (B * Y * X * C + 2 * B * D * P + 2 * B * P * C) + 12 * B * D * P     # G, prob + grad_prob, context + grad_context, geom
    rows = 4 * kept * C
    res = {"shape": name, "B": B, "D": D, "P": P, "C": C, "X": X, "Y": Y, "Z": Z, "points": B * D * P, "kept_points": kept,
           "lifted_tensor_mb": 4 * B * D * P * C / 1e6, "iters": args.iters,
           "fwd_bwd_ms": {k: {"median": med(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "speedup_median": med(times["materialised"]) / med(times["fused"]),
           "peak_alloc_mb": {k: v / 1e6 for k, v in peaks.items()},
           "grad_rel_l2_fused_vs_materialised": {"prob": diff[0], "context": diff[1]},
           "fused_kernels_us_median": {k: 1e3 * med(v) for k, v in fam.items()},
           "backward_kernel": {"us": k_us, "unique_mb": unique / 1e6, "us_at_8TBps_unique": unique / 8e12 * 1e6,
                               "gathered_row_mb": rows / 1e6, "gathered_row_TBps": rows / (k_us * 1e-6) / 1e12,
                               "row_bytes": 4 * C, "guide_infinity_cache_rows_TBps_at_1152B": 8.6,
                               "workspace_bytes": int(_lib.load().sgv3d_lift_splat_backward_workspace_bytes(B, D, P, C))}}
    print(json.dumps(res), flush=True)
    return res


CONFS = {"cfg2": (synthetic.r50_256_conf, 80), "cfg5": (synthetic.bsm_r101_256_conf, 88)}
results = []
for name in args.shapes.split(","):
    mk, C = CONFS[name]
    results.append(bench(name, mk()[0], C))
if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/lift_splat_grad_bench.py", "device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")
