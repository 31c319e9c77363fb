"""Times training the SAM ViT-B image encoder (sgv3d_amd/vit_train.py, csrc/vit_grad.hip) against the float32 torch restatement
(tests/vit_ref.py) under torch autograd on the same GPU.

    python tools/vit_train_bench.py [--out profiles/vit_train_bench.json] [--profile]

One process.  Every figure is the median of 10 HIP-event timings after 3 warm-up calls, with the device path and the baseline
ALTERNATED call by call, so that both see the same clocks and the same neighbours.

  step          forward + backward of ViT-B (random weights) at [1, 3, 576, 1024]: input tensor to the gradients of every parameter
  attention     the attention forward (with lse) + backward alone, 12 heads of 64 with both tables and padding tokens: 25 windows
                of 196 keys (a 64 x 64 map in windows of 14, padded to 70) and 4096 keys (the whole map); TFLOP/s over the
                algorithmic flops (forward 4 T^2 hd, backward 10 T^2 hd per window and head) against the f32 MFMA peak
  peak memory   torch's peak allocation over one call of each, above what was allocated before the call

``--profile``: a short run for ``rocprofv3 --kernel-trace --stats`` (three device steps, no baseline, no events).

``--dtype bf16`` (default output profiles/vit_train_bf16_bench.json): the bf16 training mode (hip_ops.VIT_TRAIN_BF16) against the
f32-tensor training path, the two ALTERNATED call by call in one process and in one compute mode (hip_ops.MFMA_BF16 with bf16 weight
gradients, which the switch needs: the only thing that differs between the two is the switch).  The same three shapes; the attention
rows report algorithmic TFLOP/s (14 T^2 hd per window and head) and executed TFLOP/s (the MFMA work the launches issue: the forward's
two products over queries padded to the query tile and keys to 32, the backward's seven over slots padded to 64) against the bf16 peak.
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
BF16_PEAK_TFLOPS = 2517.0
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


def peak_over(fn):
    """Peak allocation of one call above what is allocated before it, in MB."""
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - held) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "vit_train_bf16_bench.json" if args.dtype == "bf16" else "vit_train_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("vit_train_bench.py measures on the GPU: none is visible, and there is no CPU timing")
    import vit_ref as V
    from sgv3d_amd import vit_grad, vit_train
    from sgv3d_amd.layers.backbones.sam_encoder import build_sam_vit_b
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_sam_vit_b((864, 1536), 16).to(dev)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "pos_embed" or "rel_pos" in name:
                p.normal_(0.0, 0.02)
    params = list(model.parameters())
    x = torch.randint(0, 256, (1, 3, 576, 1024), device=dev).float()
    cot = torch.randn(1, 256, 54, 96, device=dev)

    def device_step():
        return torch.autograd.grad((vit_train.encoder_forward(model, x) * cot).sum(), params)

    if args.dtype == "bf16":
        return bench_bf16(args, model, device_step, dev)

    if args.profile:
        for _ in range(3):          # the first call also times tile candidates
            device_step()
        torch.cuda.synchronize()
        return

    names = [k for k, _ in model.named_parameters()]
    wts = {k: v.detach().clone().requires_grad_() for k, v in model.named_parameters()}
    leaves = [wts[k] for k in names]

    def torch_step():
        return torch.autograd.grad((V.encoder_forward(wts, VIT_B, x) * cot).sum(), leaves)

    result = {"gpu": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "f32_mfma_peak_tflops": F32_MFMA_PEAK_TFLOPS,
              "baseline": "tests/vit_ref.py in float32 through torch autograd on the same GPU, alternated with the device path",
              "step": [], "attention": []}
    got, ref = device_step(), torch_step()
    rel = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got, ref))
    del got, ref
    ms, ms_ref, all_ms, all_ref = timed_pair(device_step, torch_step)
    row = {"shape": [1, 3, 576, 1024], "device_ms": ms, "torch_f32_ms": ms_ref, "speedup": ms_ref / ms, "device_ms_min_max": [min(all_ms), max(all_ms)],
           "torch_ms_min_max": [min(all_ref), max(all_ref)], "device_peak_mb": peak_over(device_step), "torch_peak_mb": peak_over(torch_step),
           "worst_gradient_difference_to_torch_f32_relative_to_its_maximum": rel}
    result["step"].append(row)
    print(json.dumps(row))

    nh, hd = 12, 64
    for label, win in (("25 windows of 196 keys", (14, 14)), ("4096 keys", (64, 64))):
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(1, 64, 64, 3 * nh * hd, device=dev, generator=g).requires_grad_()
        pad = torch.randn(3 * nh * hd, device=dev, generator=g).requires_grad_()
        rh = (0.02 * torch.randn(2 * win[0] - 1, hd, device=dev, generator=g)).requires_grad_()
        rw = (0.02 * torch.randn(2 * win[1] - 1, hd, device=dev, generator=g)).requires_grad_()
        dout = torch.randn(1, 64, 64, nh * hd, device=dev, generator=g)
        leaves_a = (qkv, pad, rh, rw)
        dev_fn = lambda: torch.autograd.grad((vit_grad.attention(qkv, nh, win, pad, rh, rw) * dout).sum(), leaves_a)
        ref_fn = lambda: torch.autograd.grad((V.attention(qkv, nh, win, pad, rh, rw) * dout).sum(), leaves_a)
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(dev_fn(), ref_fn()))
        ms, ms_ref, all_ms, all_ref = timed_pair(dev_fn, ref_fn)
        nwin = -(-64 // win[0]) * -(-64 // win[1])
        t = win[0] * win[1]
        flops = nh * nwin * 14 * t * t * hd
        row = {"shape": label, "heads": nh, "head_dim": hd, "device_us": 1000.0 * ms, "torch_f32_us": 1000.0 * ms_ref, "speedup": ms_ref / ms,
               "device_us_min_max": [1000.0 * min(all_ms), 1000.0 * max(all_ms)], "torch_us_min_max": [1000.0 * min(all_ref), 1000.0 * max(all_ref)],
               "algorithmic_gflop": flops / 1e9, "algorithmic_tflops": flops / ms / 1e9,
               "share_of_f32_mfma_peak_algorithmic": flops / ms / 1e9 / F32_MFMA_PEAK_TFLOPS,
               "device_peak_mb": peak_over(dev_fn), "torch_peak_mb": peak_over(ref_fn),
               "worst_gradient_difference_to_torch_f32_relative_to_its_maximum": diff}
        result["attention"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def bench_bf16(args, model, device_step, dev):
    from sgv3d_amd import hip_ops, vit_grad
    hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.TRAIN_BF16_WGRAD = True, False, True
    assert hip_ops.vit_train_covers(768, 12) and hip_ops.vit_bf16_covers(768, 12, 3072)

    def switched(on, fn):
        def run():
            hip_ops.VIT_TRAIN_BF16 = on
            return fn()
        return run

    if args.profile:
        for _ in range(3):          # the first call also times tile candidates
            switched(True, device_step)()
        torch.cuda.synchronize()
        return
    bf_step, f32_step = switched(True, device_step), switched(False, device_step)
    result = {"gpu": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "bf16_peak_tflops": BF16_PEAK_TFLOPS,
              "baseline": "the f32-tensor training path (hip_ops.VIT_TRAIN_BF16 off) in the same compute mode (MFMA_BF16, bf16 weight "
                          "gradients), alternated with the bf16 mode call by call", "step": [], "attention": []}
    got, ref = bf_step(), f32_step()
    rel = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(got, ref))
    del got, ref
    ms, ms_ref, all_ms, all_ref = timed_pair(bf_step, f32_step)
    row = {"shape": [1, 3, 576, 1024], "bf16_ms": ms, "f32_path_ms": ms_ref, "speedup": ms_ref / ms, "bf16_ms_min_max": [min(all_ms), max(all_ms)],
           "f32_path_ms_min_max": [min(all_ref), max(all_ref)], "bf16_peak_mb": peak_over(bf_step), "f32_path_peak_mb": peak_over(f32_step),
           "worst_gradient_difference_to_the_f32_path_relative_to_its_maximum": rel}
    result["step"].append(row)
    print(json.dumps(row))

    nh, hd = 12, 64
    up = lambda v, m: -(-v // m) * m
    for label, win in (("25 windows of 196 keys", (14, 14)), ("4096 keys", (64, 64))):
        g = torch.Generator(device=dev).manual_seed(1)
        qkv = torch.randn(1, 64, 64, 3 * nh * hd, device=dev, generator=g).requires_grad_()
        pad = torch.randn(3 * nh * hd, device=dev, generator=g).requires_grad_()
        rh = (0.02 * torch.randn(2 * win[0] - 1, hd, device=dev, generator=g)).requires_grad_()
        rw = (0.02 * torch.randn(2 * win[1] - 1, hd, device=dev, generator=g)).requires_grad_()
        dout = torch.randn(1, 64, 64, nh * hd, device=dev, generator=g)
        qkv16, dout16 = qkv.detach().to(torch.bfloat16).requires_grad_(), dout.to(torch.bfloat16)
        bf_fn = lambda: torch.autograd.grad(vit_grad.attention(qkv16, nh, win, pad, rh, rw), (qkv16, pad, rh, rw), dout16)
        f32_fn2 = lambda: torch.autograd.grad(vit_grad.attention(qkv, nh, win, pad, rh, rw), (qkv, pad, rh, rw), dout)
        diff = max(float((a.float() - b).abs().max() / b.abs().max()) for a, b in zip(bf_fn(), f32_fn2()))
        ms, ms_ref, all_ms, all_ref = timed_pair(bf_fn, f32_fn2)
        nwin = -(-64 // win[0]) * -(-64 // win[1])
        t = win[0] * win[1]
        flops = nh * nwin * 14 * t * t * hd
        executed = nh * nwin * (4 * up(t, 128 if t > 64 else 64) * up(t, 32) * hd + 14 * up(t, 64) * up(t, 64) * hd)
        row = {"shape": label, "heads": nh, "head_dim": hd, "bf16_us": 1000.0 * ms, "f32_path_us": 1000.0 * ms_ref, "speedup": ms_ref / ms,
               "bf16_us_min_max": [1000.0 * min(all_ms), 1000.0 * max(all_ms)], "f32_path_us_min_max": [1000.0 * min(all_ref), 1000.0 * max(all_ref)],
               "algorithmic_gflop": flops / 1e9, "executed_gflop": executed / 1e9,
               "algorithmic_tflops": flops / ms / 1e9, "executed_tflops": executed / ms / 1e9,
               "share_of_bf16_peak_algorithmic": flops / ms / 1e9 / BF16_PEAK_TFLOPS, "share_of_bf16_peak_executed": executed / ms / 1e9 / BF16_PEAK_TFLOPS,
               "bf16_peak_mb": peak_over(bf_fn), "f32_path_peak_mb": peak_over(f32_fn2),
               "worst_gradient_difference_to_the_f32_path_relative_to_its_maximum": diff}
        result["attention"].append(row)
        print(json.dumps(row))
    hip_ops.VIT_TRAIN_BF16 = False
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
