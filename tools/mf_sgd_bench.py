#!/usr/bin/env python3
"""First measurements of MF-BPR and FunkSVD training on an MI355X: the time of one epoch on both routes of ganmf_mf_sgd_run, the
levels per batch and the launches per epoch, on the ML-1M fixture (tests/golden/Movielens1M_URM_train.npz) at batch_size 1000 and
num_factors 10 and 250.

  python tools/mf_sgd_bench.py [--reps 3] [--batch-size 1000] [--out profile_out/mf_sgd_bench.json]
  python tools/mf_sgd_bench.py --host --reference /path/to/the/reference/tree      # the reference's compiled epoch, on this host's CPU

How the numbers are taken: every timed region is a host clock around ganmf_mf_sgd_epochs(1), which blocks until the device is done.
One untimed warm-up epoch, then `reps` epochs; the median, the minimum and the maximum are reported.  The time of an epoch includes
the sampler launch, and on the levelled route the copy of the samples' ids to the host and the schedule.  The launch count is formed
on the host from the epoch's own samples (ganmf_mf_sgd_draw) with the rule of csrc/level_sched.hpp: one sampler launch, per batch one
predict launch and one update launch per level (sequential route: one).  A run without a GPU fails: there is no fallback.

--host compiles the reference's .pyx as tools/make_mf_sgd_fixture.py does (into a temporary directory) and times its epoch on the
same matrix: a host figure, from whatever CPU runs the tool."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
CASES = [("MF_BPR", False), ("FUNK_SVD", True)]


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def _train():
    train = sps.load_npz(os.path.join(GOLDEN, "Movielens1M_URM_train.npz")).tocsr().astype(np.float64)
    train.sum_duplicates()
    train.sort_indices()
    return train


def batch_levels(users, items, neg, batch_size):
    """levels of every batch of the list, by the rule of csrc/level_sched.hpp"""
    out = []
    for first in range(0, users.size, batch_size):
        lu, li, top = {}, {}, 0
        for t in range(first, min(first + batch_size, users.size)):
            u, i = int(users[t]), int(items[t])
            lv = max(lu.get(u, 0), li.get(i, 0))
            if neg is not None:
                lv = max(lv, li.get(int(neg[t]), 0))
            lv += 1
            lu[u] = li[i] = lv
            if neg is not None:
                li[int(neg[t])] = lv
            top = max(top, lv)
        out.append(top)
    return np.array(out)


def device(reps, batch_size):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    train = _train()
    rows = []
    for algorithm, use_bias in CASES:
        for k in (10, 250):
            rng = np.random.RandomState(1)
            U0, V0 = rng.normal(0.0, 0.1, (train.shape[0], k)), rng.normal(0.0, 0.1, (train.shape[1], k))
            for label, route in (("levelled", L.MF_SGD_LEVELLED), ("sequential", L.MF_SGD_SEQUENTIAL)):
                eng = Engine(train.shape[0], train.shape[1], k + 2 * int(use_bias), 1, 1, model=L.MODEL_MF)
                eng.mf_sgd_init(algorithm, train, U0, V0, use_bias=use_bias, sgd_mode="adagrad", learning_rate=float(np.float32(0.01)), seed=1)
                users, items, third = eng.mf_sgd_draw(1, 1, batch_size)      # the first timed epoch's samples
                levels = batch_levels(users, items, third if algorithm == "MF_BPR" else None, batch_size)
                n_batches = levels.size
                launches = 1 + n_batches + (int(levels.sum()) if route == L.MF_SGD_LEVELLED else n_batches)
                eng.mf_sgd_epochs(1, batch_size, route=route)      # warm-up
                ms, top = [], 0
                for _ in range(reps):
                    t0 = time.perf_counter()
                    top = max(top, eng.mf_sgd_epochs(1, batch_size, route=route))
                    ms.append((time.perf_counter() - t0) * 1e3)
                eng.close()
                row = dict(algorithm=algorithm, use_bias=use_bias, num_factors=k, route=label, epoch=_stats(ms), samples=int(users.size),
                           batches=int(n_batches), levels_mean=float(levels.mean()), levels_max=int(levels.max()), launches=int(launches),
                           us_per_launch=float(np.median(ms)) * 1e3 / launches, reported_levels=int(top))
                rows.append(row)
                print("%-8s k %3d %-10s epoch %9.2f ms (min %.2f max %.2f)  %7d samples %5d batches  levels mean %.1f max %d  %6d launches  "
                      "%.2f us/launch" % (algorithm, k, label, row["epoch"]["median_ms"], row["epoch"]["min_ms"], row["epoch"]["max_ms"],
                                          row["samples"], n_batches, row["levels_mean"], row["levels_max"], launches, row["us_per_launch"]),
                      flush=True)
    return dict(batch_size=batch_size, shape=list(train.shape), nnz=int(train.nnz), rows=rows)


def host(reference, reps, batch_size):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_mf_sgd_fixture as F
    for alias, kind in (("int", int), ("float", float), ("bool", bool)):
        if not hasattr(np, alias):
            setattr(np, alias, kind)
    sys.path.append(os.path.abspath(reference))
    scratch = tempfile.mkdtemp(prefix="mf_sgd_bench_")
    rows = []
    try:
        module = F.build_epoch_module(os.path.abspath(reference), scratch)
        train = _train()
        for algorithm, use_bias in CASES:
            for k in (10, 250):
                epoch = module.MatrixFactorization_Cython_Epoch(train.copy(), algorithm_name=algorithm, n_factors=k, learning_rate=0.01,
                                                                sgd_mode="adagrad", batch_size=batch_size, use_bias=use_bias, random_seed=1)
                epoch.epochIteration_Cython()
                ms = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    epoch.epochIteration_Cython()
                    ms.append((time.perf_counter() - t0) * 1e3)
                rows.append(dict(algorithm=algorithm, use_bias=use_bias, num_factors=k, route="reference, host CPU", epoch=_stats(ms)))
                print("%-8s k %3d reference epoch on this host's CPU: %9.2f ms (min %.2f max %.2f)" % (
                    algorithm, k, rows[-1]["epoch"]["median_ms"], rows[-1]["epoch"]["min_ms"], rows[-1]["epoch"]["max_ms"]), flush=True)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    return dict(batch_size=batch_size, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=1000)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.host and not a.reference:
        ap.error("--host needs --reference")
    doc = host(a.reference, a.reps, a.batch_size) if a.host else device(a.reps, a.batch_size)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
