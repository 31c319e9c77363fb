"""The shortcut seams of the cfg-2 image backbone (ResNet-50 at 864x1536, fp32): conv3 of a stage's first bottleneck + the shortcut
projection beside it as two launches with their per-layer choices, against the two-source launch of the f32x3 kernel
(hip_ops.conv_shortcut_x3) with each of its candidate tiles.  Every variant is captured as a hipGraph of ``--reps`` launches and the
replay is timed (best and median of ``--replays``), so host submission does not enter the figure.

    python tools/shortcut_x3_probe.py [--batch 1 8] [--out FILE.json] [--db FILE.json]

``--db``: the ``pair|shortcut|`` entries the figures imply ([1, best tile] where the fused launch is faster, else [0, 0]), to merge
into tune/gfx950_cfg2.json."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgv3d_amd import hip_ops  # noqa: E402
from sgv3d_amd.hip_ops import PackedConv  # noqa: E402

# (planes, inplanes, stride, H, W of the block's input): layer1 .. layer4 of ResNet-50 at 864 x 1536 (stem / 4)
SEAMS = ((64, 64, 1, 216, 384), (128, 256, 2, 216, 384), (256, 512, 2, 108, 192), (512, 1024, 2, 54, 96))


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
        for planes, inplanes, stride, H, W in SEAMS:
            cout = 4 * planes
            mk = lambda co, ci, **kw: PackedConv((torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5).to(dev),
                                                 scale=(torch.rand(co, generator=g) + 0.5).to(dev),
                                                 shift=(torch.randn(co, generator=g) * 0.2).to(dev), **kw)
            c3, ds = mk(cout, planes, relu=True), mk(cout, inplanes, stride=stride)
            oh, ow = ds.out_hw(H, W)
            x = torch.randn(B, H, W, inplanes, device=dev)
            mid = torch.randn(B, oh, ow, planes, device=dev)
            short, out2, out1 = (torch.empty(B, oh, ow, cout, device=dev) for _ in range(3))
            assert hip_ops.conv_shortcut_eligible(c3, ds, mid, x)
            two = lambda: c3(mid, out2, residual=ds(x, short))
            two()                                                  # (the per-layer choices: the tune DB's, or measured here)
            choices = [next(v for k, v in c._tile_cache.items()) for c in (ds, c3)]
            t2 = graph_us(two, args.reps, args.replays)
            row = {"batch": B, "seam": f"{planes}+{inplanes}->{cout} s{stride} @{H}x{W}", "two_launches_us": t2,
                   "per_layer_choices": {"shortcut": list(choices[0]), "conv3": list(choices[1])}, "fused_us": {}}
            best = None
            for t in hip_ops._shortcut_tiles(B * oh * ow, cout):
                one = lambda: hip_ops.conv_shortcut_x3(c3, ds, mid, x, out1, tile=t)
                t1 = graph_us(one, args.reps, args.replays)
                row["fused_us"][str(t)] = t1
                if best is None or t1[0] < best[1]:
                    best = (t, t1[0])
            torch.cuda.synchronize()
            row["best_fused_tile"], row["best_fused_us"] = best
            hip_ops.conv_shortcut_x3(c3, ds, mid, x, out1, tile=best[0])
            two()
            torch.cuda.synchronize()
            row["max_abs_diff"] = float((out1 - out2).abs().max())
            row["bit_equal"] = bool(torch.equal(out1, out2))
            rows.append(row)
            db[hip_ops.conv_shortcut_signature(c3, ds, x)] = [1, best[0]] if best[1] < t2[0] else [0, 0]
            print(json.dumps(row), flush=True)
            del x, mid, short, out1, out2
    for path, obj in ((args.out, {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "replays": args.replays,
                                  "times": "[best, median] microseconds per launch set, hipGraph replay", "rows": rows}), (args.db, db)):
        if path:
            with open(path, "w") as f:
                json.dump(obj, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
