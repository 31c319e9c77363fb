#!/usr/bin/env python3
"""Step A/B of the embedding distillation: ``tools/train_bench.py --dtype bf16 --graph --batch 2`` at cfg-2 with ``--distill-weight
1000`` and with 0, each run a fresh process, the two forms alternating, ``--repeats`` runs of each.  Keeps step time and
``peak_mem_gb`` of every run, the median and the spread (max - min) per form.  With the weight the model also runs its assist
convolution and that layer's backward, and the peak holds the teacher's activations of the one call ahead of the steps.  This
process never opens the GPU.
``python tools/embed_distill_step_ab.py [--out profiles/embed_distill_step_ab.json] [--repeats 3]``"""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--config", default="cfg2")
ap.add_argument("--steps", default="30", help="timed steps per run")
ap.add_argument("--timeout", type=int, default=300, help="seconds per run; a run that fails or exceeds it ends the tool")
args = ap.parse_args()
KEEP = ("config", "dtype", "graph", "batch_per_gpu", "steps", "distill_weight", "distill_frames_warped", "ms_per_step", "value", "peak_mem_gb",
        "loss", "graph_replays")
med = lambda v: sorted(v)[len(v) // 2]
base = [sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "--dtype", "bf16", "--graph", "--batch", "2", "--config", args.config,
        "--steps", args.steps, "--warmup", "3"]
res = {"tool": "tools/embed_distill_step_ab.py", "command": "python tools/train_bench.py " + " ".join(base[2:]) + " [--distill-weight 1000]",
       "runs": [], "median": {}}
for rep in range(args.repeats):
    for extra in (["--distill-weight", "1000"], []):
        out = subprocess.run(base + extra, stdout=subprocess.PIPE, timeout=args.timeout, check=True).stdout.decode()
        line = json.loads(out.strip().splitlines()[-1])
        run = {k: line[k] for k in KEEP}
        assert (run["distill_weight"] is not None) == bool(extra)
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
for on in (True, False):
    mine = [r for r in res["runs"] if (r["distill_weight"] is not None) == on]
    res["median"]["distill_1000" if on else "distill_0"] = {"ms_per_step": med([r["ms_per_step"] for r in mine]),
                                                            "spread_ms": max(r["ms_per_step"] for r in mine) - min(r["ms_per_step"] for r in mine),
                                                            "peak_mem_gb": med([r["peak_mem_gb"] for r in mine])}
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res["median"]))
