"""The four transposed convolutions of the cfg-2 SECONDFPN necks (fp32): each with its per-layer f32 choice against the f32x3
pointwise kernel's DECONV form (hip_ops.deconv_x3) with each of its candidate tiles and split-K factors.  Every variant is captured
as a hipGraph of ``--reps`` launches and the replay is timed (best and median of ``--replays``), so host submission does not enter
the figure.

    python tools/stem_deconv_probe.py [--batch 1 8] [--out FILE.json] [--db FILE.json]

``--db``: the ``pair|deconv|`` entries the figures imply ([1, 100 * split-K + best tile] where the x3 launch is faster, else
[0, 0]), to merge into tune/gfx950_cfg2.json."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgv3d_amd import hip_ops  # noqa: E402
from sgv3d_amd.hip_ops import PackedConv  # noqa: E402

# (cin, cout, ks, H, W of the level's input, channels of the concatenated map, channel offset): the image neck's 2048 -> 128 level
# at 27 x 48 and the BEV neck's 160 / 320 / 640 -> 64 levels at 128 / 64 / 32 squared
LEVELS = ((2048, 128, 2, 27, 48, 512, 384), (160, 64, 2, 128, 128, 256, 64), (320, 64, 4, 64, 64, 256, 128), (640, 64, 8, 32, 32, 256, 192))


def graph_us(fn, reps, replays):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--db", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows, db = [], {}
    for B in args.batch:
        for cin, cout, ks, H, W, y_ld, y_off in LEVELS:
            conv = PackedConv((torch.randn(cin, cout, ks, ks, generator=g) / cin ** 0.5).to(dev), stride=ks, transposed=True, relu=True,
                              scale=(torch.rand(cout, generator=g) + 0.5).to(dev), shift=(torch.randn(cout, generator=g) * 0.2).to(dev))
            x = torch.randn(B, H, W, cin, device=dev)
            out2, out1 = (torch.zeros(B, H * ks, W * ks, y_ld, device=dev) for _ in range(2))
            assert hip_ops.deconv_x3_eligible(conv, x, out1, y_off)
            old = lambda: conv(x, out2, y_coff=y_off)
            old()                                                  # (the per-layer choice: the tune DB's, or measured here)
            choice = next(v for k, v in conv._tile_cache.items())
            t2 = graph_us(old, args.reps, args.replays)
            row = {"batch": B, "level": f"{cin}->{cout} k{ks} @{H}x{W}", "f32_us": t2, "per_layer_choice": list(choice), "x3_us": {}}
            best = None
            for t, splits in hip_ops._deconv_x3_candidates(B * H * W, ks * ks * cout, cin // 32):
                for sk in splits:
                    one = lambda: hip_ops.deconv_x3(conv, x, out1, y_off, tile=t, split_k=sk)
                    t1 = graph_us(one, args.reps, args.replays)
                    row["x3_us"][f"{t}.{sk}"] = t1
                    if best is None or t1[0] < best[2]:
                        best = (t, sk, t1[0])
            torch.cuda.synchronize()
            row["best_x3"], row["best_x3_us"] = [best[0], best[1]], best[2]
            hip_ops.deconv_x3(conv, x, out1, y_off, tile=best[0], split_k=best[1])
            old()
            torch.cuda.synchronize()
            row["max_abs_diff"] = float((out1 - out2).abs().max())
            row["output_scale"] = float(out2.abs().max())
            rows.append(row)
            db[hip_ops.deconv_x3_signature(conv, x)] = [1, 100 * best[1] + best[0]] if best[2] < t2[0] else [0, 0]
            print(json.dumps(row), flush=True)
            del x, out1, out2
    for path, obj in ((args.out, {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "replays": args.replays,
                                  "times": "[best, median] microseconds per launch, hipGraph replay", "rows": rows}), (args.db, db)):
        if path:
            with open(path, "w") as f:
                json.dump(obj, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
