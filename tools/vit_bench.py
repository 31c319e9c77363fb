"""Times the SAM ViT-B image encoder on the device path against the float32 torch restatement (tests/vit_ref.py) on the same GPU.

    python tools/vit_bench.py [--out profiles/vit_bench.json] [--profile]
    python tools/vit_bench.py --dtype bf16 [--out profiles/vit_bf16_bench.json] [--profile]

One process.  Every figure is the median of 10 HIP-event timings after 3 warm-up calls, with the device path and the
baseline ALTERNATED call by call, so that both see the same clocks and the same neighbours.

  forward       ViT-B (random weights) at [1, 3, 576, 1024] and at batch 4: the whole forward, input tensor to output map
  attention     the attention launch alone at its two workload shapes, 12 heads of 64: 25 windows of 196 keys (a 64 x 64 map in
                windows of 14, padded to 70) and 4096 keys (the whole map); TFLOP/s over the EXECUTED flops (every 64 x 64
                tile the kernel multiplies, masked slots included, and the two rel-pos table products) and over the
                ALGORITHMIC flops (4 T^2 hd per window and head), against the 157.3 TFLOP/s f32 MFMA peak bench.py uses

``--dtype bf16``: the encoder's bf16 mode (hip_ops.MFMA_BF16 and hip_ops.VIT_BF16 on) against the f32 DEVICE path of the same process
(both switches off: the default path), alternated call by call in the same way: the forward at both batch sizes with the agreement
of the two outputs, and sgv3d_vit_attention_bf16 against sgv3d_vit_attention at the two attention shapes, TFLOP/s against the bf16
MFMA peak (16 x the f32 one).

``--profile``: a short run for ``rocprofv3 --kernel-trace --stats`` (four device forwards at batch 1, no baseline, no events).
With ``SGV3D_TUNE_CACHE=<file of an earlier --save-tune run>`` no tile candidates are timed and the trace holds the forwards only.
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

F32_MFMA_PEAK_TFLOPS = 157.3
BF16_MFMA_PEAK_TFLOPS = 16 * F32_MFMA_PEAK_TFLOPS
WARMUP, REPEATS = 3, 10
VIT_B = dict(img_size=1024, patch_size=16, embed_dim=768, depth=12, num_heads=12, out_chans=256, window_size=14,
             global_attn_indexes=[2, 5, 8, 11], eps=1e-6, final_dim=(864, 1536), downsample_factor=16)


def timed_pair(a, b):
    """Median milliseconds of ``a`` and of ``b``, alternated."""
    for _ in range(WARMUP):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPEATS):
        for fn, acc in ((a, ta), (b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return statistics.median(ta), statistics.median(tb), ta, tb


def attention_flops(b, h, w, nh, hd, win):
    """(executed, algorithmic) flops of one sgv3d_vit_attention launch with both rel-pos tables."""
    nwin = -(-h // win[0]) * -(-w // win[1])
    t = win[0] * win[1]
    tiles = -(-t // 64)
    table_rows = sum(16 * -(-(2 * s - 1) // 16) for s in win)
    blocks = b * nh * nwin * tiles
    executed = blocks * (tiles * 2 * (2 * 64 * 64 * hd) + 2 * 64 * table_rows * hd)
    algorithmic = b * nh * nwin * (4 * t * t * hd + 2 * t * (win[0] + win[1]) * hd)
    return executed, algorithmic


def attention_flops_bf16(b, h, w, nh, hd, win):
    """(executed, algorithmic) flops of one sgv3d_vit_attention_bf16 launch with both rel-pos tables: a workgroup multiplies its 64 or
    128 queries (csrc/vit_bf16.hip: 128 where a window has more than 64 slots and the LDS of two workgroups fits) with every live
    32-key block, Q K^T over the head dimension padded to a multiple of 32."""
    nwin = -(-h // win[0]) * -(-w // win[1])
    t = win[0] * win[1]
    kv_bytes = 2 * 64 * ((2 * hd + 16) + (96 if hd == 32 else 160))
    wide = t > 64 and kv_bytes + 128 * 4 * ((win[0] | 1) + (win[1] | 1)) <= 64 * 1024
    qt = 128 if wide else 64
    hd_qk = 32 * -(-hd // 32)
    table_rows = sum(16 * -(-(2 * s - 1) // 16) for s in win)
    blocks = b * nh * nwin * -(-t // qt)
    executed = blocks * (-(-t // 32) * 2 * qt * 32 * (hd_qk + hd) + 2 * qt * table_rows * hd_qk)
    algorithmic = b * nh * nwin * (4 * t * t * hd + 2 * t * (win[0] + win[1]) * hd)
    return executed, algorithmic


def main_bf16(args, model, dev):
    """The bf16 mode against the f32 device path of this process."""
    from sgv3d_amd import hip_ops
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b, vit_attention, vit_attention_bf16

    def mode(bf16):
        hip_ops.MFMA_BF16 = hip_ops.VIT_BF16 = bf16

    if args.profile:
        mode(True)
        x = torch.randint(0, 256, (1, 3, 576, 1024), device=dev).float()
        for _ in range(4):          # without a tune cache the first call also times tile candidates
            model(x)
        torch.cuda.synchronize()
        return
    # one module per mode (each packs its weights once), the same parameters
    model_f32 = build_sam_vit_b((864, 1536), 16).to(dev).eval()
    model_f32.load_state_dict(model.state_dict())

    def run(m, bf16, x):
        mode(bf16)
        return m(x)

    result = {"gpu": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "bf16_mfma_peak_tflops": BF16_MFMA_PEAK_TFLOPS,
              "f32_mfma_peak_tflops": F32_MFMA_PEAK_TFLOPS,
              "baseline": "the f32 device path of the same process (MFMA_BF16 and VIT_BF16 off), alternated with the bf16 mode",
              "forward": [], "attention": []}
    for batch in (1, 4):
        x = torch.randint(0, 256, (batch, 3, 576, 1024), device=dev).float()
        ref = run(model_f32, False, x).clone()
        got = run(model, True, x).clone()
        assert all(b.bf16_mode() for b in model.blocks)
        err = (got - ref).double()
        ms, ms_ref, all_ms, all_ref = timed_pair(lambda: run(model, True, x), lambda: run(model_f32, False, x))
        result["forward"].append({"shape": [batch, 3, 576, 1024], "bf16_ms": ms, "f32_ms": ms_ref, "speedup": ms_ref / ms,
                                  "bf16_ms_min_max": [min(all_ms), max(all_ms)], "f32_ms_min_max": [min(all_ref), max(all_ref)],
                                  "max_abs_diff_to_f32": float(err.abs().max()), "rel_l2_diff_to_f32": float(err.norm() / ref.double().norm()),
                                  "output_rms": float(ref.double().pow(2).mean().sqrt()), "images_per_s": 1000.0 * batch / ms})
        print(json.dumps(result["forward"][-1]))

    nh, hd = 12, 64
    for label, win in (("25 windows of 196 keys", (14, 14)), ("4096 keys", (64, 64))):
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(1, 64, 64, 3 * nh * hd, device=dev, generator=g)
        pad = torch.randn(3 * nh * hd, device=dev, generator=g)
        rh = 0.02 * torch.randn(2 * win[0] - 1, hd, device=dev, generator=g)
        rw = 0.02 * torch.randn(2 * win[1] - 1, hd, device=dev, generator=g)
        qkv16 = qkv.to(torch.bfloat16)
        out = torch.empty(1, 64, 64, nh * hd, device=dev)
        out16 = torch.empty(1, 64, 64, nh * hd, device=dev, dtype=torch.bfloat16)
        diff = float((vit_attention_bf16(qkv16, nh, win, pad, rh, rw).float() - vit_attention(qkv, nh, win, pad, rh, rw)).abs().max())
        ms, ms_ref, all_ms, all_ref = timed_pair(lambda: vit_attention_bf16(qkv16, nh, win, pad, rh, rw, out=out16),
                                                 lambda: vit_attention(qkv, nh, win, pad, rh, rw, out=out))
        executed, algorithmic = attention_flops_bf16(1, 64, 64, nh, hd, win)
        row = {"shape": label, "heads": nh, "head_dim": hd, "bf16_us": 1000.0 * ms, "f32_us": 1000.0 * ms_ref, "speedup": ms_ref / ms,
               "bf16_us_min_max": [1000.0 * min(all_ms), 1000.0 * max(all_ms)], "f32_us_min_max": [1000.0 * min(all_ref), 1000.0 * max(all_ref)],
               "executed_gflop": executed / 1e9, "algorithmic_gflop": algorithmic / 1e9, "executed_tflops": executed / ms / 1e9,
               "algorithmic_tflops": algorithmic / ms / 1e9,
               "share_of_bf16_mfma_peak_executed": executed / ms / 1e9 / BF16_MFMA_PEAK_TFLOPS,
               "share_of_bf16_mfma_peak_algorithmic": algorithmic / ms / 1e9 / BF16_MFMA_PEAK_TFLOPS, "max_abs_diff_to_f32": diff}
        result["attention"].append(row)
        print(json.dumps(row))
    mode(False)
    out_path = args.out or os.path.join(ROOT, "profiles", "vit_bf16_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)
    if args.save_tune:
        hip_ops.save_tune_db(args.save_tune)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="default profiles/vit_bench.json (--dtype bf16: profiles/vit_bf16_bench.json)")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--save-tune", help="write the per-layer tile choices this run measured (SGV3D_TUNE_CACHE=<file> replays them)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vit_bench.py measures on the GPU: none is visible, and there is no CPU timing")
    import vit_ref as V
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b, vit_attention
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_sam_vit_b((864, 1536), 16).to(dev).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "pos_embed" or "rel_pos" in name:
                p.normal_(0.0, 0.02)
    if args.dtype == "bf16":
        return main_bf16(args, model, dev)
    args.out = args.out or os.path.join(ROOT, "profiles", "vit_bench.json")
    if args.profile:
        x = torch.randint(0, 256, (1, 3, 576, 1024), device=dev).float()
        for _ in range(4):          # without a tune cache the first call also times tile candidates
            model(x)
        torch.cuda.synchronize()
        return

    wts = {k: v.detach() for k, v in model.state_dict().items()}
    result = {"gpu": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "f32_mfma_peak_tflops": F32_MFMA_PEAK_TFLOPS,
              "baseline": "tests/vit_ref.py in float32 through torch on the same GPU, alternated with the device path",
              "forward": [], "attention": []}
    for batch in (1, 4):
        x = torch.randint(0, 256, (batch, 3, 576, 1024), device=dev).float()
        with torch.no_grad():
            ref = V.encoder_forward(wts, VIT_B, x)
            got = model(x)
            diff = float((got - ref).abs().max())
            ms, ms_ref, all_ms, all_ref = timed_pair(lambda: model(x), lambda: V.encoder_forward(wts, VIT_B, x))
        result["forward"].append({"shape": [batch, 3, 576, 1024], "device_ms": ms, "torch_f32_ms": ms_ref, "speedup": ms_ref / ms,
                                  "device_ms_min_max": [min(all_ms), max(all_ms)], "torch_ms_min_max": [min(all_ref), max(all_ref)],
                                  "max_abs_diff_to_torch_f32": diff, "images_per_s": 1000.0 * batch / ms})
        print(json.dumps(result["forward"][-1]))

    nh, hd = 12, 64
    for label, win in (("25 windows of 196 keys", (14, 14)), ("4096 keys", (64, 64))):
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(1, 64, 64, 3 * nh * hd, device=dev, generator=g)
        pad = torch.randn(3 * nh * hd, device=dev, generator=g)
        rh = 0.02 * torch.randn(2 * win[0] - 1, hd, device=dev, generator=g)
        rw = 0.02 * torch.randn(2 * win[1] - 1, hd, device=dev, generator=g)
        out = torch.empty(1, 64, 64, nh * hd, device=dev)
        diff = float((vit_attention(qkv, nh, win, pad, rh, rw) - V.attention(qkv, nh, win, pad, rh, rw)).abs().max())
        ms, ms_ref, all_ms, _ = timed_pair(lambda: vit_attention(qkv, nh, win, pad, rh, rw, out=out),
                                           lambda: V.attention(qkv, nh, win, pad, rh, rw))
        executed, algorithmic = attention_flops(1, 64, 64, nh, hd, win)
        row = {"shape": label, "heads": nh, "head_dim": hd, "device_us": 1000.0 * ms, "torch_f32_us": 1000.0 * ms_ref,
               "device_us_min_max": [1000.0 * min(all_ms), 1000.0 * max(all_ms)], "executed_gflop": executed / 1e9,
               "algorithmic_gflop": algorithmic / 1e9, "executed_tflops": executed / ms / 1e9,
               "algorithmic_tflops": algorithmic / ms / 1e9, "share_of_f32_mfma_peak_executed": executed / ms / 1e9 / F32_MFMA_PEAK_TFLOPS,
               "max_abs_diff_to_torch_f32": diff}
        result["attention"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if args.save_tune:
        from sgv3d_amd import hip_ops
        hip_ops.save_tune_db(args.save_tune)


if __name__ == "__main__":
    main()
