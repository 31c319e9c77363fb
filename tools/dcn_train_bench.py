#!/usr/bin/env python3
"""Layer A/B of the differentiable fused deformable convolution in the mixed-precision training mode: forward + backward of
``misc_grad.deform_conv3x3`` against the column form it replaces (``misc_grad.deform_im2col3x3`` + one 1x1 ``conv_grad.conv2d`` per
group + ``torch.cat``), the latter in default mode (float-atomic sampling adjoint) and in deterministic mode (gather adjoint), at
the HeightNet DCN of cfg-2 batch 2 (2 x 54 x 96 x 512, 4 groups) and cfg-3 batch 4 (4 x 68 x 120 x 512).

Timing: HIP events in this process, the three forms alternating, after warm-up; median and max - min per form; the launches of
each form alone from the events ``hip_ops.prof`` puts around them; peak allocation of each form over forward + backward.
``python tools/dcn_train_bench.py [--out profiles/dcn_train_bench.json] [--iters 10]``"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgv3d_amd import _lib, conv_grad, hip_ops, misc_grad

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--shapes", default="cfg2_b2,cfg3_b4")
args = ap.parse_args()
dev = torch.device("cuda")
# every switch the three forms read, pinned: the mode of tools/train_bench.py --dtype bf16
hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.BF16_ACTIVATIONS = True, False, False
hip_ops.DCN_FUSED = hip_ops.DCN_FUSED_BF16 = hip_ops.TRAIN_BF16_WGRAD = True
hip_ops.AUTOTUNE = False                      # the library's rules for every convolution: no first-call timing inside the timed region
SWITCHES = {k: getattr(hip_ops, k) for k in ("MFMA_BF16", "MFMA_F32X3", "BF16_ACTIVATIONS", "DCN_FUSED", "DCN_FUSED_BF16", "TRAIN_BF16_WGRAD",
                                             "AUTOTUNE", "WGRAD_BF16_ALLTAPS")}
SHAPES = {"cfg2_b2": (2, 54, 96, 512, 4, 512), "cfg3_b4": (4, 68, 120, 512, 4, 512)}
med = lambda v: sorted(v)[len(v) // 2]


def column_form(x, offset, weight, g):
    cout, cpg = int(weight.shape[0]), int(weight.shape[1])
    opg = cout // g
    col = misc_grad.deform_im2col3x3(x, offset, g)
    outs = []
    for gi in range(g):
        wg = weight[gi * opg:(gi + 1) * opg].permute(0, 2, 3, 1).reshape(opg, 9 * cpg, 1, 1)
        outs.append(conv_grad.conv2d(col[..., gi * 9 * cpg:(gi + 1) * 9 * cpg].contiguous(), wg))
    return torch.cat(outs, -1)


def bench(name):
    B, H, W, C, g, cout = SHAPES[name]
    P, cpg = B * H * W, C // g
    gen = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.randn(B, H, W, C, device=dev, generator=gen)
    off0 = torch.randn(B, H, W, 18, device=dev, generator=gen)
    w0 = torch.randn(cout, cpg, 3, 3, device=dev, generator=gen) / (9 * cpg) ** 0.5
    dy = torch.randn(B, H, W, cout, device=dev, generator=gen)
    forms = {"fused": (lambda a, b, c: misc_grad.deform_conv3x3(a, b, c, g), False),
             "column_default": (lambda a, b, c: column_form(a, b, c, g), False),
             "column_deterministic": (lambda a, b, c: column_form(a, b, c, g), True)}

    def once(key, ev=None):
        fn, det = forms[key]
        hip_ops.DETERMINISTIC = det
        leaves = [t.detach().requires_grad_(True) for t in (x0, off0, w0)]
        if ev:
            ev[0].record()
        fn(*leaves).backward(dy)
        if ev:
            ev[1].record()
        return [t.grad for t in leaves]

    def peak(key):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        once(key)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - start

    peaks = {k: peak(k) for k in forms}
    gf, gd = once("fused"), once("column_deterministic")
    torch.cuda.synchronize()
    same = {"dx_equal": bool(torch.equal(gf[0], gd[0])), "doffset_equal": bool(torch.equal(gf[1], gd[1])),
            "dw_rel_l2": float((gf[2] - gd[2]).norm() / gd[2].norm())}
    for _ in range(args.warmup):
        for k in forms:
            once(k)
    times = {k: [] for k in forms}
    for _ in range(args.iters):                     # alternating: the forms see the same clocks and cache state
        for k in forms:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            once(k, ev)
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    launches = {}
    for k in forms:                                 # the launches of each form alone (events around every launch)
        hip_ops.PROFILE = []
        for _ in range(args.iters):
            once(k)
        torch.cuda.synchronize()
        fam = {}
        for rec in hip_ops.PROFILE:
            fam.setdefault(rec[0].split('|')[0], []).append(rec[2].elapsed_time(rec[3]))
        hip_ops.PROFILE = None
        # (a label launched n times per pass: n x the median launch)
        launches[k] = {lab: {"per_pass": len(v) // args.iters, "us_per_pass": 1e3 * med(v) * (len(v) // args.iters)} for lab, v in fam.items()}
    hip_ops.DETERMINISTIC = False
    flop = 2.0 * P * C * 9 * (cout // g)
    unique = 4.0 * (P * (C + 18 + cout) + cout * cpg * 9)
    nws = int(_lib.load().sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes(B, H, W, C, g, cout // g, 0))
    wg_us = launches["fused"]["dcn_wgrad_bf16"]["us_per_pass"]
    res = {"shape": name, "B": B, "H": H, "W": W, "C": C, "groups": g, "cout": cout, "pixels": P, "column_tensor_mb": 4.0 * P * 9 * C / 1e6,
           "iters": args.iters, "fwd_bwd_ms": {k: {"median": med(v), "spread": max(v) - min(v), "min": min(v)} for k, v in times.items()},
           "peak_alloc_mb": {k: v / 1e6 for k, v in peaks.items()}, "fused_vs_column_deterministic": same, "launches_us": launches,
           "weight_gradient": {"fused_us": wg_us, "column_form_us": launches["column_default"].get("conv_wgrad_bf16", {}).get("us_per_pass"),
                               "split": nws // (9 * cout * cpg * 4), "workspace_mb": nws / 1e6, "flop": flop,
                               "us_at_2.5PFLOPs": flop / 2.5e15 * 1e6, "unique_hbm_mb": unique / 1e6, "us_at_8TBps_unique": unique / 8e12 * 1e6,
                               "gathered_corner_mb": 4.0 * P * 9 * C * 4 / 1e6}}
    print(json.dumps(res), flush=True)
    return res


results = [bench(n) for n in args.shapes.split(",")]
if args.out:
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/dcn_train_bench.py", "device": torch.cuda.get_device_name(0), "switches": SWITCHES, "results": results}, f, indent=1)
        f.write("\n")
