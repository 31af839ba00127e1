"""Prediction cosine-similarity study (ganmf_score_similarity) wall time at the ML-1M shape: 6040 users x 3706 items, k = 250,
all users.  Usage: python tools/similarity_bench.py [--reps 7] [--skip-host]

Times, alternating in one process (median of --reps repeats, host wall time around calls that end in a stream synchronise):

  * the device call in three forms -- statistics only, with pool = 512 block means, with the full [6040, 6040] matrix;
  * the host route on the same box: _compute_item_score (scores to the host), float32 row normalisation and float32 S^ @ S^.T in
    numpy, np.mean and np.std -- what AblationStudy.py:88-92 does through sklearn;

for both arithmetic candidates of the Gram product (GANMF_TUNE=gram=1, the default: exact three-way bf16 split, gram=0: plain fp32 MFMA; one
engine each), and reads the Gram launch's device time from the library's profile (ganmf_profile_read) for its achieved TFLOP/s
against the fp32 MFMA roof.  One JSON line per arithmetic."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_ROOF_TFLOPS = 157.3      # MI355X, dense fp32 matrix peak

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--skip-host", action="store_true", help="device forms only")
args = ap.parse_args()

NU, NI, K = 6040, 3706, 250
rng = np.random.RandomState(0)
U = (rng.standard_normal((NU, K)) / np.sqrt(K)).astype(np.float32)
V = rng.standard_normal((NI, K)).astype(np.float32)
users = np.arange(NU, dtype=np.int32)


def host_route(eng):
    s = eng.scores(users)
    norm = np.sqrt(np.einsum("ij,ij->i", s, s))
    norm[norm == 0.0] = 1.0
    s /= norm[:, None]
    c = s @ s.T
    return float(np.mean(c)), float(np.std(c))


def median_ms(fns, reps):
    times = {name: [] for name, _ in fns}
    for name, fn in fns:
        fn()                                              # warm-up: code objects, buffers, the split of V
    for _ in range(reps):                                 # alternating
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)) for name, t in times.items()}


for arith, label in ((0, "fp32 MFMA"), (1, "bf16 x 3 split")):
    os.environ["GANMF_TUNE"] = "gram=%d" % arith
    from ganmf_amd.engine import Engine
    eng = Engine(NU, NI, K, 16, 32)
    eng.set_tensor(100, U)
    eng.set_tensor(101, V)
    fns = [("stats_only", lambda: eng.score_similarity(users)),
           ("pool_512", lambda: eng.score_similarity(users, pool=512)),
           ("full_matrix", lambda: eng.score_similarity(users, return_matrix=True))]
    if not args.skip_host and arith == 0:
        fns.append(("host_route", lambda: host_route(eng)))
    res = median_ms(fns, args.reps)
    got = eng.score_similarity(users)
    eng.profile(True)
    for _ in range(5):
        eng.score_similarity(users)
    prof = {e["name"]: e for e in eng.profile_read()}
    eng.profile(False)
    gram = [e for name, e in prof.items() if name.startswith("gram_similarity")][0]
    gram_ms = gram["ms"] / gram["launches"]
    out = {"shape": "ml1m", "users": NU, "items": NI, "k": K, "arithmetic": label, "reps": args.reps,
           "mean": got["mean"], "std": got["std"],
           "gram_launch_ms": round(gram_ms, 4), "gram_tflops": round(gram["flops"] / gram["launches"] / gram_ms * 1e-9, 1),
           "fp32_mfma_roof_tflops": FP32_MFMA_ROOF_TFLOPS}
    for name, (med, lo, hi) in res.items():
        out[name + "_ms"] = med
        out[name + "_ms_min_max"] = [lo, hi]
    if "host_route" in res:
        out["host_mean_std"] = list(host_route(eng))
        out["host_over_stats_only"] = round(res["host_route"][0] / res["stats_only"][0], 1)
    print(json.dumps(out), flush=True)
    eng.close()
