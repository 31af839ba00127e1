#!/usr/bin/env python3
"""A/B runs of bench.py under different environments: steps/s and the per-class launch averages that changed.
usage: tools/ab.py "NAME=VALUE ..." "NAME=VALUE ..." [--reps N] [--class SUBSTRING] [--save DIR]    ("" = default environment)
--save DIR keeps every run's JSON line as DIR/rep<r>_<i>.json (i = position of the environment on the command line).  A run that fails or
takes longer than ten minutes ends the tool with exit code 1: nothing more is started on the GPU behind a run that went wrong."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
reps, cls = 2, None
if "--reps" in args:
    i = args.index("--reps"); reps = int(args[i + 1]); del args[i:i + 2]
save = None
if "--save" in args:
    i = args.index("--save"); save = args[i + 1]; del args[i:i + 2]
    os.makedirs(save, exist_ok=True)
if "--class" in args:
    i = args.index("--class"); cls = args[i + 1]; del args[i:i + 2]
for rep in range(reps):
    for pos, spec in enumerate(args):
        env = dict(os.environ)
        for kv in spec.split():
            k, v = kv.split("=", 1)
            env[k] = v
        try:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600)
            d = json.loads(out.stdout.strip().splitlines()[-1])
        except subprocess.TimeoutExpired:
            print("%-50s TIMED OUT" % (spec or "(default)"))
            sys.exit(1)
        except Exception:
            print("%-50s FAILED (exit %d): %s" % (spec or "(default)", out.returncode, out.stderr[-300:]))
            sys.exit(1)
        if save:
            open(os.path.join(save, "rep%d_%d.json" % (rep, pos)), "w").write(json.dumps(d) + "\n")
        extra = ""
        if cls:
            extra = "  ".join("%s:%s %.2f us" % (k.get("step", "?"), k["name"][:28], k["avg_us"]) for k in d["kernels"] if cls in k["name"])
        print("%-50s %8.1f steps/s  D %8.1f  G %8.1f  fn %.3f  %s" % (spec or "(default)", d["value"], d.get("d_steps_per_s", 0), d.get("g_steps_per_s", 0), d["roofline"].get("frac", 0), extra), flush=True)
