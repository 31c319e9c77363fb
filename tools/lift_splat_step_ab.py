#!/usr/bin/env python3
"""Step A/B of the differentiable fused lift-splat: ``tools/train_bench.py --dtype bf16 --graph --batch 2`` with and without
``--no-fuse-lift-splat`` at cfg-2 and cfg-5, each run a fresh process, the two forms alternating, ``--repeats`` runs of each.
Keeps step time and ``peak_mem_gb`` of every run and the median per form.  This process never opens the GPU.
``python tools/lift_splat_step_ab.py [--out profiles/lift_splat_train_bench.json] [--repeats 3]``"""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--configs", default="cfg2,cfg5")
ap.add_argument("--steps", default="30,20", help="timed steps per config")
ap.add_argument("--timeout", type=int, default=300, help="seconds per run; a run that fails or exceeds it ends the tool")
args = ap.parse_args()
KEEP = ("config", "dtype", "graph", "batch_per_gpu", "steps", "fuse_lift_splat", "ms_per_step", "value", "peak_mem_gb", "loss", "graph_replays")
med = lambda v: sorted(v)[len(v) // 2]
res = {"tool": "tools/lift_splat_step_ab.py", "runs": [], "median": {}}
for cfg, steps in zip(args.configs.split(","), args.steps.split(",")):
    base = [sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "--dtype", "bf16", "--graph", "--batch", "2", "--config", cfg,
            "--steps", steps, "--warmup", "3"]
    res.setdefault("commands", {})[cfg] = " ".join(["python"] + [os.path.relpath(a, ROOT) if a.startswith(ROOT) else a for a in base[1:]]) + " [--no-fuse-lift-splat]"
    for rep in range(args.repeats):
        for extra in ([], ["--no-fuse-lift-splat"]):
            out = subprocess.run(base + extra, stdout=subprocess.PIPE, timeout=args.timeout, check=True).stdout.decode()
            line = json.loads(out.strip().splitlines()[-1])
            run = {k: line[k] for k in KEEP}
            assert run["fuse_lift_splat"] == (not extra)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    for fused in (True, False):
        mine = [r for r in res["runs"] if r["config"] == cfg and r["fuse_lift_splat"] == fused]
        res["median"][f"{cfg}_{'fused' if fused else 'two_step'}"] = {"ms_per_step": med([r["ms_per_step"] for r in mine]),
                                                                     "peak_mem_gb": med([r["peak_mem_gb"] for r in mine])}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
print(json.dumps(res["median"]))
