#!/usr/bin/env python3
"""First measurements of CAAE training on an MI355X, at the ML-1M shape with the hyper-parameters the reference's search found
(experiments/CAAE__1M/best_params.txt, typed in below as settings): the time of one epoch (ganmf_caae_epoch with the device sampler)
and of its parts -- the order, both generators over all users and both CDFs; one discriminator pass; the generator steps -- and MAP@5
on the golden ML-1M test split after the settings' 95 epochs on the train split.  The only reference-side figures are its own log's
22 h 20 min for 50 trials and MAP@5 0.0898 (experiments/CAAE__1M/results.txt, on its validation split).

  python tools/caae_bench.py [--reps 3] [--seeds 1 2] [--out profiles/caae_fit.md]

How the numbers are taken: every region is a host clock around a call that blocks until the device is done (the ganmf_caae_* entries
synchronise their stream before they return); one untimed warm-up call, then `reps` calls, median (minimum - maximum).  An epoch call
always forms the order and both CDFs, so "one discriminator pass" and "the generator steps" are the calls with only those steps minus
the call with none.  Nothing here is asserted anywhere: the file records what was measured.  A run without a GPU fails: there is no
fallback."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

SETTINGS = dict(epochs=95, d_steps=10, g_steps=10, gpr_steps=20, g_layers=5, gpr_layers=4, g_units=100, gpr_units=150, num_factors=43,
                m_batch=64, d_bsize=9216, lr=0.001, beta=0.1, S=0.6, lmbda=0.9)
LOGGED_MAP5_VALIDATION = 0.0898      # experiments/CAAE__1M/results.txt


def _timed(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return np.median(ms), "%.1f (%.1f - %.1f)" % (np.median(ms), np.min(ms), np.max(ms))


def measure(train, reps):
    from ganmf_amd.CAAE import CAAE
    hp = SETTINGS
    model = CAAE(train, seed=1, is_experiment=True)
    model._build(hp["num_factors"], hp["g_layers"], hp["g_units"], d_bsize=hp["d_bsize"], m_batch=hp["m_batch"], lmbda=hp["lmbda"],
                 beta=hp["beta"], lr=hp["lr"], S=hp["S"])
    model._init_weights()
    eng = model.engine
    state = {"e": 0}

    def epoch(d, g, p):
        state["e"] += 1
        eng.caae_epoch(state["e"], d, g, p)
    row = {"n_s": model.n_s}
    row["front"] = _timed(lambda: epoch(0, 0, 0), reps)
    row["d_pass"] = _timed(lambda: epoch(1, 0, 0), reps)
    row["g_steps"] = _timed(lambda: epoch(0, hp["g_steps"], hp["gpr_steps"]), reps)
    row["epoch"] = _timed(lambda: epoch(hp["d_steps"], hp["g_steps"], hp["gpr_steps"]), reps)
    eng.close()
    return row


def accuracy(train, test, seeds):
    from ganmf_amd.CAAE import CAAE
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    out = []
    for seed in seeds:
        model = CAAE(train, seed=seed, is_experiment=True)
        t0 = time.perf_counter()
        model.fit(allow_worse=None, **SETTINGS)
        secs = time.perf_counter() - t0
        out.append((seed, secs, float(EvaluatorHoldoutFast(test, [5]).evaluateRecommender(model)[0][5]["MAP"]),
                    float(model.train_d_loss[-1]), float(model.train_pg_loss[-1]), float(model.train_ng_loss[-1])))
        model.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    load = lambda name: sps.load_npz(os.path.join(GOLDEN, name)).tocsr().astype(np.float32)
    train, test = load("Movielens1M_URM_train.npz"), load("Movielens1M_URM_test.npz")
    hp = SETTINGS
    r = measure(train, a.reps)
    front, d_pass, g_steps, epoch = (r[k][0] for k in ("front", "d_pass", "g_steps", "epoch"))
    slices = -(-train.nnz // hp["d_bsize"])
    lines = ["# CAAE on an MI355X: the epoch, its parts, and MAP@5 on ML-1M", "",
             "`python tools/caae_bench.py --reps %d` on one MI355X; the ML-1M train split of `tests/golden` (%d users, %d items, %d"
             % (a.reps, train.shape[0], train.shape[1], train.nnz),
             "interactions) and the hyper-parameters of the reference's `experiments/CAAE__1M/best_params.txt` (typed into the tool):",
             "d_steps %d, g_steps %d, gpr_steps %d, %d layers of %d units, %d factors, d_bsize %d (%d slices, two steps each), m_batch %d,"
             % (hp["d_steps"], hp["g_steps"], hp["gpr_steps"], hp["g_layers"], hp["g_units"], hp["num_factors"], hp["d_bsize"], slices,
                hp["m_batch"]),
             "n_s = %d policy draws per row.  Milliseconds, median (minimum - maximum): a host clock around `ganmf_caae_epoch` calls, which"
             % r["n_s"],
             "block until the device is done.  Recorded, not asserted.", "",
             "| call | ms |", "|---|---|",
             "| epoch with no step: the order, G and G' over all users, both CDFs | %s |" % r["front"][1],
             "| ... with one discriminator pass (%d steps) | %s |" % (2 * slices, r["d_pass"][1]),
             "| ... with the generator steps (%d of G, %d of G') and no pass | %s |" % (hp["g_steps"], hp["gpr_steps"], r["g_steps"][1]),
             "| the whole epoch (%d passes, %d + %d steps) | %s |" % (hp["d_steps"], hp["g_steps"], hp["gpr_steps"], r["epoch"][1]), "",
             "By difference: one discriminator pass %.1f ms (%.1f us per step), the generator steps %.1f ms (%.2f ms per step); %.3f"
             % (d_pass - front, 1e3 * (d_pass - front) / (2 * slices), g_steps - front, (g_steps - front) / (hp["g_steps"] + hp["gpr_steps"]),
                epoch / 1e3),
             "seconds per epoch.  The reference logs 22 h 20 min for the 50 trials of its search on this data set (of up to 300 epochs",
             "each, with early stopping): no per-epoch figure of its own exists to set beside this one.", ""]
    print("\n".join(lines), flush=True)
    if a.seeds:
        lines += ["## MAP@5", "",
                  "`fit()` with these settings (95 epochs, no early stopping, the device sampler) on the train split, evaluated with",
                  "`EvaluatorHoldoutFast` at cut-off 5 on the test split.  The reference's search logs MAP@5 = %.4f for these settings on"
                  % LOGGED_MAP5_VALIDATION,
                  "its validation split after training on train_small, from its own initialisation, numpy's stream and early stopping:",
                  "another split and another protocol, set here only for scale.", "",
                  "| seed | fit seconds | MAP@5 test (train) | last epoch's mean D loss | G loss | G' loss |", "|---|---|---|---|---|---|"]
        for row in accuracy(train, test, a.seeds):
            lines.append("| %d | %.1f | %.7f | %.5g | %.5g | %.5g |" % row)
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
