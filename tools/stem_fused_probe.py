"""The cfg-2 image stem (fp32, 3 x 864 x 1536 -> 216 x 384 x 64): the three launches -- ``nchw_to_nhwc(c_pad=4)``, the 7x7 / stride 2
convolution, ``maxpool3x3s2`` -- with the committed per-layer (f32 MFMA) choice for the convolution and with the f32x3 tap-major kernel
on each of its 64-channel and 128-channel tiles, against the one-launch stem (hip_ops.stem_fused) with each of its variants.  Every
form is captured as a hipGraph of ``--reps`` repetitions and the replay is timed (best and median of ``--replays``), so host
submission does not enter the figure.

    python tools/stem_fused_probe.py [--batch 1 8] [--hw 864 1536] [--out FILE.json] [--db FILE.json]

``--db``: the ``pair|stem|`` entries the figures imply ([1, best variant] where the fused launch beats the three launches with the
committed choice, else [0, 0]), to merge into tune/gfx950_cfg2.json."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgv3d_amd import hip_ops  # noqa: E402
from sgv3d_amd.hip_ops import PackedConv  # noqa: E402
from tools.stem_deconv_probe import graph_us  # noqa: E402

X3_TILES = (60, 61, 62, 64, 65, 66)             # conv_pw_x3_kernel: {32, 64, 128} pixels x {128, 64} channels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--hw", type=int, nargs=2, default=[864, 1536])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--db", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    H, W = args.hw
    conv = PackedConv((torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5).to(dev), stride=2, pad=3, relu=True, cin_pad=4,
                      scale=(torch.rand(64, generator=g) + 0.5).to(dev), shift=(torch.randn(64, generator=g) * 0.2).to(dev))
    rows, db = [], {}
    for B in args.batch:
        x = torch.randn(B, 3, H, W, device=dev)
        assert hip_ops.stem_fused_eligible(conv, x)
        hc, wc = conv.out_hw(H, W)
        hp, wp = hip_ops.stem_fused_out_hw(H, W)
        x4 = torch.empty(B, H, W, 4, device=dev)
        mid = torch.empty(B, hc, wc, 64, device=dev)
        out3, out1 = (torch.zeros(B, hp, wp, 64, device=dev) for _ in range(2))

        def three(tile=None):
            hip_ops.nchw_to_nhwc(x, c_pad=4, out=x4)
            if tile is None:
                conv(x4, mid)
            else:
                conv(x4, mid, tile=tile, split_k=1)
            hip_ops.maxpool3x3s2(mid, out=out3)
        three()                                                    # (the per-layer choice: the tune DB's, or measured here)
        choice = next(v for k, v in conv._tile_cache.items() if k[0] == B)
        row = {"batch": B, "image": f"3x{H}x{W}", "per_layer_choice": list(choice), "three_launches_us": graph_us(three, args.reps, args.replays),
               "three_launches_x3_us": {}, "fused_us": {}}
        for t in X3_TILES:
            row["three_launches_x3_us"][str(t)] = graph_us(lambda: three(t), args.reps, args.replays)
        three(65)
        torch.cuda.synchronize()
        x3_map = out3.clone()
        best = None
        for v in hip_ops.STEM_FUSED_VARIANTS:
            t1 = graph_us(lambda: hip_ops.stem_fused(conv, x, out1, variant=v), args.reps, args.replays)
            row["fused_us"][str(v)] = t1
            if best is None or t1[0] < best[1]:
                best = (v, t1[0])
            torch.cuda.synchronize()
            assert torch.equal(out1, x3_map), f"variant {v} differs from the three launches on the f32x3 kernel"
        three()
        torch.cuda.synchronize()
        row["best_fused"], row["best_fused_us"] = best[0], best[1]
        row["bit_equal_to_x3_three_launches"] = True
        row["max_abs_diff_to_committed_f32_stem"] = float((out1 - out3).abs().max())
        row["output_scale"] = float(out3.abs().max())
        rows.append(row)
        db[hip_ops.stem_fused_signature(conv, x)] = [1, best[0]] if best[1] < row["three_launches_us"][0] else [0, 0]
        print(json.dumps(row), flush=True)
        del x, x4, mid, out1, out3
    for path, obj in ((args.out, {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "replays": args.replays,
                                  "times": "[best, median] microseconds per repetition, hipGraph replay", "rows": rows}), (args.db, db)):
        if path:
            with open(path, "w") as f:
                json.dump(obj, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
