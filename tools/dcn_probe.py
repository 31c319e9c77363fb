#!/usr/bin/env python3
"""Dev probe: the deformable 3x3 convolution of HeightNet (lss_fpn.py:190-198; cfg-2: 512 -> 512, groups 4, 54x96; cfg-3 at
batch 4: 68x120) as deform_im2col3x3 + one GEMM per group (rounds 1-4) against the one-launch forms, each as a hipGraph of 10:

  f32 mode    sgv3d_deform_conv3x3_forward (csrc/dcn_fused.hip), median of 7 replays
  bf16 mode   sgv3d_deform_conv3x3_forward_bf16 (csrc/dcn_fused_bf16.hip), bf16 and f32 input tensors: best and spread of 5
              replays of either form -> profiles/dcn_bf16_bench.json

  python tools/dcn_probe.py [f32|bf16|all]      (default f32; only bf16 / all write the JSON)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgv3d_amd import hip_ops                            # noqa: E402
from sgv3d_amd.hip_ops import PackedConv                 # noqa: E402
from tools.vp_probe3 import graph_us                     # noqa: E402

SHAPES = (("cfg-2 512 g4 @54x96", 1, 512, 54, 96, 4), ("cfg-3 b4 512 g4 @68x120", 4, 512, 68, 120, 4))
BF16_PEAK_TFLOPS = 2500.0


def graph_repeats_us(fn, reps=10, repeats=5):
    """``fn`` captured ``reps`` times into one hipGraph; microseconds per call of each of ``repeats`` timed replays."""
    dev = torch.device("cuda")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    ts = []
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                fn()
        g.replay()
        side.synchronize()
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            g.replay()
            e1.record(side)
            side.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    torch.cuda.current_stream(dev).wait_stream(side)
    return ts


def f32_mode():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    for name, B, C, H, W, groups in SHAPES:
        cpg = C // groups
        x = torch.randn(B, H, W, C, generator=g).to(dev)
        off = (torch.randn(B, H, W, 18, generator=g) * 1.5).to(dev)
        weight = torch.randn(C, cpg, 3, 3, generator=g) / (9 * cpg) ** 0.5
        convs = [PackedConv(weight[gi * cpg:(gi + 1) * cpg].permute(0, 2, 3, 1).reshape(cpg, 9 * cpg, 1, 1).contiguous().to(dev))
                 for gi in range(groups)]
        out_a = torch.empty(B, H, W, C, device=dev)
        out_b = torch.empty(B, H, W, C, device=dev)

        def old():
            col = hip_ops.deform_im2col3x3(x, off, groups)
            for gi, conv in enumerate(convs):
                conv(col, out_a, x_coff=gi * 9 * cpg, y_coff=gi * cpg)

        def new():
            hip_ops.deform_conv3x3(x, off, convs, out=out_b)
        old(); new()
        torch.cuda.synchronize()
        err = float((out_a - out_b).abs().max()) / float(out_a.abs().max())
        flop = 2.0 * B * H * W * C * 9 * cpg
        t_old, t_new = graph_us(old, reps=10), graph_us(new, reps=10)
        print(f"{name:26s} im2col + {groups} GEMMs {t_old:7.1f} us | fused {t_new:7.1f} us = {flop / t_new / 1e6:6.1f} TFLOP/s "
              f"({flop / t_new / 1e6 / 157.3:.2f} of the f32 MFMA peak) | rel. difference {err:.1e}", flush=True)


def bf16_mode(out_path):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    # every switch the comparison depends on is pinned (an inherited SGV3D_F32X3 / SGV3D_DCN_FUSED / SGV3D_NO_BF16_ACTIVATIONS would
    # change what the "im2col form" is) and the resulting switch_state() goes into the JSON
    pinned = {"MFMA_BF16": True, "MFMA_F32X3": False, "DCN_FUSED": True, "DCN_FUSED_BF16": True, "BF16_ACTIVATIONS": True}
    saved = {k: getattr(hip_ops, k) for k in pinned}
    for k, v in pinned.items():
        setattr(hip_ops, k, v)
    switches = [str(v) for v in hip_ops.switch_state()]
    rows = []
    try:
        for name, B, C, H, W, groups in SHAPES:
            cpg = C // groups
            x32 = torch.randn(B, H, W, C, generator=g).to(dev)
            off = (torch.randn(B, H, W, 18, generator=g) * 1.5).to(dev)
            weight = torch.randn(C, cpg, 3, 3, generator=g) / (9 * cpg) ** 0.5
            convs = [PackedConv(weight[gi * cpg:(gi + 1) * cpg].permute(0, 2, 3, 1).reshape(cpg, 9 * cpg, 1, 1).contiguous().to(dev))
                     for gi in range(groups)]
            packed = hip_ops.PackedDeformBf16(weight.to(dev), groups)
            flop = 2.0 * B * H * W * C * 9 * cpg
            for x in (x32.bfloat16(), x32):
                out_a = torch.empty(B, H, W, C, dtype=x.dtype, device=dev)
                out_b = torch.empty(B, H, W, C, dtype=x.dtype, device=dev)

                def old():
                    col = hip_ops.deform_im2col3x3(x, off, groups)
                    for gi, conv in enumerate(convs):
                        conv(col, out_a, x_coff=gi * 9 * cpg, y_coff=gi * cpg)

                def new():
                    hip_ops.deform_conv3x3_bf16(x, off, packed, out=out_b)
                old(); new()
                torch.cuda.synchronize()
                err = float((out_a.float() - out_b.float()).abs().max()) / float(out_a.float().abs().max())
                t_old, t_new = graph_repeats_us(old), graph_repeats_us(new)
                row = {"shape": name, "batch": B, "channels": C, "h": H, "w": W, "groups": groups,
                       "x_dtype": str(x.dtype).replace("torch.", ""), "graph_calls": 10, "repeats": 5,
                       "im2col_form_us": [round(t, 2) for t in t_old], "one_launch_us": [round(t, 2) for t in t_new],
                       "im2col_form_best_us": round(min(t_old), 2), "one_launch_best_us": round(min(t_new), 2),
                       "im2col_form_spread_us": round(max(t_old) - min(t_old), 2), "one_launch_spread_us": round(max(t_new) - min(t_new), 2),
                       "one_launch_tflops": round(flop / min(t_new) / 1e6, 1),
                       "one_launch_fraction_of_bf16_peak": round(flop / min(t_new) / 1e6 / BF16_PEAK_TFLOPS, 3),
                       "mfma_floor_us": round(flop / BF16_PEAK_TFLOPS / 1e6, 1),
                       "max_rel_difference": err}
                row["one_launch_faster_beyond_spread"] = bool(
                    min(t_old) - min(t_new) > max(row["im2col_form_spread_us"], row["one_launch_spread_us"]))
                rows.append(row)
                print(f"{name:26s} x {row['x_dtype']:8s} im2col + {groups} GEMMs {min(t_old):7.1f} us (spread {row['im2col_form_spread_us']:.1f}) | "
                      f"one launch {min(t_new):7.1f} us (spread {row['one_launch_spread_us']:.1f}) = {row['one_launch_tflops']:6.1f} TFLOP/s "
                      f"({row['one_launch_fraction_of_bf16_peak']:.3f} of the bf16 peak) | rel. difference {err:.1e}", flush=True)
    finally:
        for k, v in saved.items():
            setattr(hip_ops, k, v)
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump({"tool": "tools/dcn_probe.py bf16", "device": torch.cuda.get_device_name(0), "bf16_peak_tflops": BF16_PEAK_TFLOPS,
                       "switch_state": switches, "rows": rows}, f, indent=1)
            f.write("\n")
    return rows


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "f32"          # no argument: the f32 comparison, as before; writes no file
    if mode in ("f32", "all"):
        f32_mode()
    if mode in ("bf16", "all"):
        bf16_mode(os.environ.get("SGV3D_DCN_PROBE_OUT", os.path.join(ROOT, "profiles", "dcn_bf16_bench.json")))


if __name__ == "__main__":
    main()
