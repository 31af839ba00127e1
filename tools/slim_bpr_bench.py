#!/usr/bin/env python3
"""First measurements of SLIM-BPR training on an MI355X: the time of one epoch on both routes of ganmf_slim_bpr_run, the number of
levels per epoch, the time per sample of the sequential walk, and ganmf_slim_bpr_finish, on the ML-1M train_small fixture
(6040 users, 3706 items: an epoch is 6041 samples).

  python tools/slim_bpr_bench.py [--reps 5] [--epochs 4] [--topk 200] [--out profile_out/slim_bpr_bench.json]
  python tools/slim_bpr_bench.py --trials [--seeds 5] [--write]     # the logged trials of tests/golden/slim_bpr_trial_logs_ml1m.json

How the numbers are taken: every timed region is a host clock around a call that blocks until the device is done
(ganmf_slim_bpr_epochs and ganmf_slim_bpr_finish synchronise their stream before they return).  One untimed warm-up call, then `reps`
calls of `epochs` epochs each; the median, the minimum and the maximum of the per-epoch time are reported.  The time of an epoch
includes the sampler launch, and on the levelled route the copy of the samples' items to the host and the schedule.  A run without a
GPU fails: there is no fallback.

--trials: every logged trial is fitted with `seeds` seeds of ours (1, 2, ...) for its logged number of epochs plus 25 -- the reference
trains with early stopping (a validation every 5 epochs, 5 allowed without improvement), logs the epoch of the best validation and
evaluates the model of the LAST epoch, 25 epochs later -- and MAP@5 on the validation split is printed next to the logged value;
--write stores mean, standard deviation and the bound of the test (3 standard deviations) in the fixture."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "slim_bpr_trial_logs_ml1m.json")
sys.path.insert(0, ROOT)


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def _engine(train):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(train.shape[0], train.shape[1], 1, 1, 1, model=L.MODEL_ITEMSIM)
    eng.set_confidence(0, train)
    eng.set_seen(train)
    return eng


def timing(reps, epochs, topk):
    from ganmf_amd import _lib as L
    train = sps.load_npz(os.path.join(GOLDEN, "Movielens1M_URM_train_small.npz")).tocsr().astype(np.float32)
    train.sort_indices()
    per_epoch = train.shape[0] + 1
    rows = []
    for label, symmetric, route in (("sequential, dense S", False, L.SLIM_SEQUENTIAL), ("levelled, dense S", False, L.SLIM_LEVELLED),
                                    ("sequential, symmetric S", True, L.SLIM_SEQUENTIAL)):
        for mode in ("sgd", "adagrad", "adam"):
            eng = _engine(train)
            eng.slim_bpr_init(symmetric=symmetric, sgd_mode=mode, learning_rate=0.01, lambda_i=1e-5, lambda_j=1e-5, seed=1)
            eng.slim_bpr_epochs(1, mode=route)      # warm-up
            ms, levels = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                levels.append(eng.slim_bpr_epochs(epochs, mode=route))
                ms.append((time.perf_counter() - t0) * 1e3 / epochs)
            t0 = time.perf_counter()
            nnz = eng.slim_bpr_finish(topk)
            first = (time.perf_counter() - t0) * 1e3
            fin = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng.slim_bpr_finish(topk)
                fin.append((time.perf_counter() - t0) * 1e3)
            eng.close()
            row = dict(route=label, sgd_mode=mode, epoch=_stats(ms), us_per_sample=float(np.median(ms)) * 1e3 / per_epoch,
                       levels_per_epoch=float(np.mean(levels)) / epochs, finish=_stats(fin), finish_first_ms=first, topk=topk, nnz=nnz)
            rows.append(row)
            print("%-24s %-8s epoch %8.2f ms (min %.2f max %.2f)  %6.2f us/sample  %7.1f levels/epoch  finish(topK %d) %.2f ms, nnz %d"
                  % (label, mode, row["epoch"]["median_ms"], row["epoch"]["min_ms"], row["epoch"]["max_ms"], row["us_per_sample"],
                     row["levels_per_epoch"], topk, row["finish"]["median_ms"], nnz), flush=True)
    return dict(samples_per_epoch=per_epoch, n_items=train.shape[1], epochs_per_call=epochs, rows=rows)


def trials(n_seeds, write):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from ganmf_amd.SLIM_BPR import SLIM_BPR_Cython
    doc = json.load(open(FIXTURE))
    train = sps.load_npz(os.path.join(GOLDEN, doc["train"])).tocsr()
    ev = EvaluatorHoldoutFast(sps.load_npz(os.path.join(GOLDEN, doc["validation"])).tocsr(), [doc["at"]])
    for t in doc["trials"]:
        p = dict(t["params"])
        p["epochs"] += doc["epochs_after_best"]
        values, secs = [], []
        for seed in range(1, n_seeds + 1):
            model = SLIM_BPR_Cython(train.copy())
            t0 = time.perf_counter()
            model.fit(random_seed=seed, **p)
            secs.append(time.perf_counter() - t0)
            values.append(float(ev.evaluateRecommender(model)[0][doc["at"]][doc["metric"]]))
            model.engine.close()
        mean, std = float(np.mean(values)), float(np.std(values, ddof=1))
        t.update(seeds=list(range(1, n_seeds + 1)), values=values, mean=mean, std=std, bound=3.0 * std)
        print("%-7s symmetric %-5s topK %4d epochs %3d + %d: logged %.7f  ours mean %.7f std %.2e  |logged - seed 1| %.2e  bound %.2e  %s"
              "  (fit %.1f s)" % (p["sgd_mode"], p["symmetric"], p["topK"], t["params"]["epochs"], doc["epochs_after_best"], t["logged"], mean,
                                  std, abs(values[0] - t["logged"]), 3.0 * std, "inside" if abs(values[0] - t["logged"]) <= 3.0 * std else "OUTSIDE",
                                  float(np.median(secs))), flush=True)
    if write:
        json.dump(doc, open(FIXTURE, "w"), indent=1)
        print("wrote", FIXTURE)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--topk", type=int, default=200)
    ap.add_argument("--trials", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = trials(a.seeds, a.write) if a.trials else timing(a.reps, a.epochs, a.topk)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
