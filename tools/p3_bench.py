#!/usr/bin/env python3
"""First measurements of P3alphaRecommender / RP3betaRecommender on an MI355X: the fit through the class and its passes by profile
class, and the hold-out evaluation, on the ML-1M train / test fixtures at the reference's tuned P3alpha parameters (the `best` row of
tests/golden/p3_trial_logs_ml1m.json, the reference's experiments/P3alphaRecommender__1M/best_params.txt; RP3beta: the same with its
default beta = 0.6).

  python tools/p3_bench.py [--reps 7] [--out profile_out/p3_bench.json]
  python tools/p3_bench.py --reference /path/to/reference      # CPU only: the reference's Python classes on the same fits

How the numbers are taken: every timed region is a host clock around a call that ends in a device synchronise (ganmf_p3_fit blocks;
evaluateRecommender returns metric values).  One untimed warm-up, then `reps` repetitions; the median, the minimum and the maximum
are reported.  fit() includes the host's part (the transition weights in float64, a new handle, three uploads of the matrix); the
classes are ganmf_profile_read of one further, profiled ganmf_p3_fit (hipEvent brackets around the kernels, a run of its own).  A run
without a GPU fails: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TRAIN, TEST = "Movielens1M_URM_train.npz", "Movielens1M_URM_test.npz"


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def _timed(fn, reps, warm=True):
    if warm:
        fn()      # warm-up: code objects, buffers
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stats(out)


def _settings():
    doc = json.load(open(os.path.join(GOLDEN, "p3_trial_logs_ml1m.json")))
    best = [t["params"] for t in doc["trials"] if t["role"] == "best"][0]
    return [("P3alpha", dict(best)), ("RP3beta", dict(best, beta=0.6))]


def device_bench(reps):
    sys.path.insert(0, ROOT)
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from ganmf_amd.P3 import P3alphaRecommender, RP3betaRecommender, transition_terms
    train = sps.load_npz(os.path.join(GOLDEN, TRAIN)).tocsr()
    test = sps.load_npz(os.path.join(GOLDEN, TEST)).tocsr()
    rows = []
    for name, p in _settings():
        model = (P3alphaRecommender if name == "P3alpha" else RP3betaRecommender)(train)
        fit = _timed(lambda: model.fit(**p), reps)
        ev = EvaluatorHoldoutFast(test, [5, 10, 20])
        evaluate = _timed(lambda: ev.evaluateRecommender(model), reps)
        results, _ = ev.evaluateRecommender(model)
        # the entry alone, and its launches by class: the uploads are in place, one profiled call, a run of its own
        rs, pui, cs = transition_terms(train, p["alpha"], p.get("beta"))
        k = min(p["topK"], model.n_items)
        model.engine.set_confidence(1, pui)
        entry = _timed(lambda: model.engine.p3_fit(k, rs, col_scale=cs, normalize=p["normalize_similarity"], col_topk=k), reps)
        model.engine.profile(True)
        nnz = model.engine.p3_fit(k, rs, col_scale=cs, normalize=p["normalize_similarity"], col_topk=k)
        classes = model.engine.profile_read()
        model.engine.profile(False)
        row = dict(model=name, users=train.shape[0], items=train.shape[1], nnz=int(train.nnz), params=p, w_nnz=int(nnz),
                   evaluated_users=len(ev.usersToEvaluate), fit=fit, p3_fit_entry=entry, evaluate=evaluate,
                   fit_device_ms=float(sum(c["ms"] for c in classes)), fit_classes=classes, MAP_at_5=float(results[5]["MAP"]))
        rows.append(row)
        print("%-8s %5d x %5d nnz %7d topK %4d: fit() %.1f ms, ganmf_p3_fit %.1f ms (kernels %.1f ms), evaluate %.1f ms, MAP@5 %.6f" % (
            name, train.shape[0], train.shape[1], train.nnz, p["topK"], fit["median_ms"], entry["median_ms"], row["fit_device_ms"],
            evaluate["median_ms"], row["MAP_at_5"]), flush=True)
        for c in classes:
            print("    %-44s %4d launches %9.3f ms" % (c["name"], c["launches"], c["ms"]))
        model.engine.close()
    return rows


def reference_bench(reference, reps):
    """the reference's own Python classes on the CPU, same matrix and parameters"""
    sys.path.insert(0, os.path.abspath(reference))      # (this repository is not on the path: its GraphBased/ would be preferred)
    for alias, kind in (("int", int), ("float", float), ("bool", bool), ("object", object)):
        if alias not in np.__dict__:      # aliases the reference still uses, removed in numpy 1.24
            setattr(np, alias, kind)
    from GraphBased.P3alphaRecommender import P3alphaRecommender
    from GraphBased.RP3betaRecommender import RP3betaRecommender
    train = sps.load_npz(os.path.join(GOLDEN, TRAIN)).tocsr()
    rows = []
    for name, p in _settings():
        cls = P3alphaRecommender if name == "P3alpha" else RP3betaRecommender
        stats = _timed(lambda: cls(train.copy()).fit(**p), reps, warm=False)
        rows.append(dict(model=name, reference_python_fit=stats))
        print("%-8s reference Python fit on the CPU: median %.0f ms (min %.0f, max %.0f, %d reps)" % (
            name, stats["median_ms"], stats["min_ms"], stats["max_ms"], reps), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None, help="path of the reference tree: time its Python classes on the CPU instead")
    a = ap.parse_args()
    rows = reference_bench(a.reference, a.reps) if a.reference else device_bench(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
