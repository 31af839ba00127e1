#!/usr/bin/env python3
"""First measurements of CFGAN training on an MI355X, at the ML-1M shape with the hyper-parameters the reference's search found
(experiments/CFGAN_user_1M and CFGAN_item_1M, typed in below as settings): the time of one epoch (ganmf_cfgan_epoch with the device
sampler), of its discriminator passes and generator passes alone, and of the sampler alone; beside them the epoch of the float32 numpy
restatement (tests/helpers_cfgan.py) on this box's CPUs and the host numpy sampler (draw_masks_numpy); and MAP@5 of user-mode fits on
the golden ML-1M split beside the reference's logged values (0.1332 on the validation split after training on train_small, the
protocol of its search; 0.3066 on the test split after training on the whole train split, its final run).

  python tools/cfgan_bench.py [--reps 5] [--out profiles/cfgan_fit.md]

How the numbers are taken: every device region is a host clock around a call that blocks until the device is done (the ganmf_cfgan_*
entries synchronise their stream before they return); one untimed warm-up call, then `reps` calls, median (minimum - maximum).  The
CPU figures are one warm-up and `cpu_reps` timed runs under whatever thread count numpy's BLAS takes from the environment.  Nothing
here is asserted anywhere: the file records what was measured.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

SETTINGS = {
    "user": dict(epochs=26, d_steps=1, g_steps=1, d_layers=1, g_layers=3, d_hidden_act="linear", g_hidden_act="tanh", scheme="ZR",
                 d_batch_size=128, g_batch_size=512, zr_ratio=0.8358867527625552, zp_ratio=0.4790322061823805, zr_coefficient=1.0,
                 d_lr=0.006667224996558187, g_lr=0.0001, d_reg=1.4368667306633583e-06, g_reg=4.355218606865685e-05, d_nodes=4,
                 g_nodes=637),
    "item": dict(epochs=96, d_steps=5, g_steps=3, d_layers=3, g_layers=1, d_hidden_act="sigmoid", g_hidden_act="linear", scheme="PM",
                 d_batch_size=256, g_batch_size=256, zr_ratio=0.20305542251107173, zp_ratio=0.6629766293162644,
                 zr_coefficient=0.9715229767080295, d_lr=0.0008592758651155475, g_lr=0.00010927957465307145,
                 d_reg=3.3858309892774854e-06, g_reg=1.14202213234902e-05, d_nodes=154, g_nodes=519),
}
LOGGED_MAP5_USER = 0.1332259            # experiments/CFGAN_user_1M/results.txt: the search's best validation MAP@5
LOGGED_MAP5_USER_TEST = 0.3065821       # test_results/CFGAN_user_1M/test_results.txt:1


def _timed(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return "%.2f (%.2f - %.2f)" % (np.median(ms), np.min(ms), np.max(ms))


def measure(mode, train, reps, cpu_reps):
    from ganmf_amd.CFGAN import CFGAN, draw_masks_numpy, init_weights, non_interactions
    from tests.helpers_cfgan import CFGANRef
    hp = dict(SETTINGS[mode])
    model = CFGAN(train, mode=mode, seed=1, is_experiment=True)
    model._build(hp["d_nodes"], hp["d_layers"], hp["g_nodes"], hp["g_layers"], hp["d_hidden_act"], hp["g_hidden_act"], scheme=hp["scheme"],
                 d_batch_size=hp["d_batch_size"], g_batch_size=hp["g_batch_size"], zr_ratio=hp["zr_ratio"],
                 zr_coefficient=hp["zr_coefficient"], d_lr=hp["d_lr"], g_lr=hp["g_lr"], d_reg=hp["d_reg"], g_reg=hp["g_reg"])
    model._init_weights()
    eng = model.engine
    state = {"e": 0}

    def epoch(d, g, draw):
        state["e"] += 1
        eng.cfgan_epoch(state["e"], d, g, draw=draw)
    row = dict(mode=mode, rows=model.num_users, cols=model.num_items)
    row["epoch"] = _timed(lambda: epoch(hp["d_steps"], hp["g_steps"], True), reps)
    row["d_pass"] = _timed(lambda: epoch(1, 0, False), reps)
    row["g_pass"] = _timed(lambda: epoch(0, 1, False), reps)
    row["sampler"] = _timed(lambda: eng.cfgan_draw_masks(state["e"]), reps)
    eng.close()
    fitm = model._URM_fit
    free = non_interactions(fitm)
    row["numpy_sampler"] = _timed(lambda: draw_masks_numpy(fitm, hp["scheme"], hp["zr_ratio"], rng=np.random.RandomState(1), free=free), cpu_reps)
    zr, pm = draw_masks_numpy(fitm, hp["scheme"], hp["zr_ratio"], rng=np.random.RandomState(1), free=free)
    C = fitm.toarray()
    ref = CFGANRef(init_weights(1, model.num_items, hp["d_nodes"], hp["d_layers"], hp["g_nodes"], hp["g_layers"]), d_act=hp["d_hidden_act"],
                   g_act=hp["g_hidden_act"], d_lr=hp["d_lr"], g_lr=hp["g_lr"], d_reg=hp["d_reg"], g_reg=hp["g_reg"],
                   zr_coefficient=hp["zr_coefficient"], dtype=np.float32)
    row["numpy_epoch"] = _timed(lambda: ref.epoch(C, pm, zr, hp["d_steps"], hp["g_steps"], hp["d_batch_size"], hp["g_batch_size"]), cpu_reps)
    return row


def accuracy(train_small, train, validation, test):
    """per seed: (seed, fit seconds, MAP@5 on validation after a fit on train_small, MAP@5 on test after a fit on train)"""
    from ganmf_amd.CFGAN import CFGAN
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    hp = dict(SETTINGS["user"])
    out = []
    for seed in (1, 2, 3):
        vals, secs = [], []
        for fit_on, held_out in ((train_small, validation), (train, test)):
            model = CFGAN(fit_on, mode="user", seed=seed, is_experiment=True)
            t0 = time.perf_counter()
            model.fit(allow_worse=None, **hp)
            secs.append(time.perf_counter() - t0)
            vals.append(float(EvaluatorHoldoutFast(held_out, [5]).evaluateRecommender(model)[0][5]["MAP"]))
            model.engine.close()
        out.append((seed, float(np.mean(secs)), vals[0], vals[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    load = lambda name: sps.load_npz(os.path.join(GOLDEN, name)).tocsr().astype(np.float32)
    train, validation, test = load("Movielens1M_URM_train.npz"), load("Movielens1M_URM_validation.npz"), load("Movielens1M_URM_test.npz")
    train_small = load("Movielens1M_URM_train_small.npz")
    lines = ["# CFGAN on an MI355X: the epoch, its passes, the mask sampler, and MAP@5 on ML-1M", "",
             "`python tools/cfgan_bench.py --reps %d` on one MI355X; the ML-1M train split of `tests/golden` (%d users, %d items, %d"
             % (a.reps, train.shape[0], train.shape[1], train.nnz),
             "interactions) and the hyper-parameters of the reference's `experiments/CFGAN_user_1M` / `CFGAN_item_1M` (typed into the tool).",
             "Milliseconds, median (minimum - maximum): a host clock around calls that block until the device is done; the CPU columns are the",
             "float32 numpy restatement of `tests/helpers_cfgan.py` and `draw_masks_numpy` (non-interaction lists formed once, outside the",
             "clock) on the same box with OMP_NUM_THREADS=%s.  Recorded, not asserted." % os.environ.get("OMP_NUM_THREADS", "unset"), "",
             "| mode | rows x columns | d_steps / g_steps | epoch | one D pass | one G pass | device sampler | numpy epoch (CPU) | numpy sampler (CPU) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for mode in ("user", "item"):
        r = measure(mode, train, a.reps, a.cpu_reps)
        hp = SETTINGS[mode]
        lines.append("| %s | %d x %d | %d / %d | %s | %s | %s | %s | %s | %s |" % (mode, r["rows"], r["cols"], hp["d_steps"], hp["g_steps"], r["epoch"],
                     r["d_pass"], r["g_pass"], r["sampler"], r["numpy_epoch"], r["numpy_sampler"]))
        print(lines[-1], flush=True)
    lines += ["", "## MAP@5, user mode", "",
              "`fit()` with the user-mode settings (26 epochs, no early stopping, the device mask sampler), evaluated with",
              "`EvaluatorHoldoutFast` at cut-off 5: on the validation split after a fit on `train_small` (the protocol of the reference's",
              "search, which logs MAP@5 = %.7f for these settings) and on the test split after a fit on the whole train split (its final" % LOGGED_MAP5_USER,
              "run logs %.7f).  The reference's figures come from its own initialisation, numpy's mask stream and early stopping." % LOGGED_MAP5_USER_TEST,
              "", "| seed | fit seconds | MAP@5 validation (train_small) | MAP@5 test (train) |", "|---|---|---|---|"]
    for seed, secs, v, t in accuracy(train_small, train, validation, test):
        lines.append("| %d | %.1f | %.7f | %.7f |" % (seed, secs, v, t))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
