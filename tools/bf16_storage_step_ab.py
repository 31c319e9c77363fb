#!/usr/bin/env python3
"""Step A/B of bf16 activation storage in the image backbone: ``tools/train_bench.py --dtype bf16 --graph --batch 2`` at cfg-2 with
``--act-storage f32`` and ``--act-storage bf16``, each run a fresh process, the two storages alternating, ``--repeats`` runs of each.
Keeps step time and ``peak_mem_gb`` of every run, the median and the spread (max - min) per storage.  This process never opens the GPU.
``python tools/bf16_storage_step_ab.py [--out profiles/bf16_storage_train_bench.json] [--repeats 3]``"""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--config", default="cfg2")
ap.add_argument("--steps", default="30", help="timed steps per run")
ap.add_argument("--timeout", type=int, default=300, help="seconds per run; a run that fails or exceeds it ends the tool")
args = ap.parse_args()
KEEP = ("config", "dtype", "graph", "batch_per_gpu", "steps", "act_storage", "ms_per_step", "value", "peak_mem_gb", "loss", "graph_replays")
med = lambda v: sorted(v)[len(v) // 2]
base = [sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "--dtype", "bf16", "--graph", "--batch", "2", "--config", args.config,
        "--steps", args.steps, "--warmup", "3"]
res = {"tool": "tools/bf16_storage_step_ab.py", "command": "python tools/train_bench.py " + " ".join(base[2:]) + " --act-storage {f32,bf16}",
       "runs": [], "median": {}}
for rep in range(args.repeats):
    for storage in ("f32", "bf16"):
        out = subprocess.run(base + ["--act-storage", storage], stdout=subprocess.PIPE, timeout=args.timeout, check=True).stdout.decode()
        line = json.loads(out.strip().splitlines()[-1])
        run = {k: line[k] for k in KEEP}
        assert run["act_storage"] == storage, run
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
for storage in ("f32", "bf16"):
    mine = [r for r in res["runs"] if r["act_storage"] == storage]
    ms = [r["ms_per_step"] for r in mine]
    res["median"][storage] = {"ms_per_step": med(ms), "spread_ms": max(ms) - min(ms), "peak_mem_gb": med([r["peak_mem_gb"] for r in mine])}
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(json.dumps(res["median"]))
