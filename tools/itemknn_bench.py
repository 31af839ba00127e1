#!/usr/bin/env python3
"""First measurements of ItemKNNCFRecommender on an MI355X: the fit and the full hold-out evaluation through the class, on the
ML-1M, LastFM and hetrec2011 fixtures at each dataset's tuned cosine parameters (tests/golden/itemknn_best_params_cosine.json, the
reference's experiments/ItemKNNCFRecommender_cosine_<dataset>/best_params.txt), with the launches by profile class.

  python tools/itemknn_bench.py [--reps 7] [--out profile_out/itemknn_bench.json]
  python tools/itemknn_bench.py --reference /path/to/reference      # CPU only: the reference's Python class on the same fits

How the numbers are taken: every timed region is a host clock around a call that ends in a device synchronise (fit() returns after
ganmf_itemknn_fit has copied the column counts back; evaluateRecommender returns metric values).  One untimed warm-up per shape, then
`reps` repetitions; the median, the minimum and the maximum are reported.  fit() includes the host's part (CSC conversion, norms,
two uploads of the matrix, creating the handle); `fit_device_ms` is the sum of the profile classes of one further, profiled fit
(hipEvent brackets around the kernels, a run of its own).  A run without a GPU fails: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
DATASETS = {"ml1m": ("Movielens1M_URM_train.npz", "Movielens1M_URM_test.npz"), "lastfm": ("LastFM_URM_train.npz", "LastFM_URM_test.npz"),
            "hetrec2011": ("hetrec2011_URM_train.npz", "hetrec2011_URM_test.npz")}


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def _timed(fn, reps):
    fn()      # warm-up: code objects, buffers
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stats(out)


def device_bench(reps):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender
    params = json.load(open(os.path.join(GOLDEN, "itemknn_best_params_cosine.json")))
    rows = []
    for name, (train_file, test_file) in DATASETS.items():
        train = sps.load_npz(os.path.join(GOLDEN, train_file)).tocsr()
        test = sps.load_npz(os.path.join(GOLDEN, test_file)).tocsr()
        p = params[name]
        model = ItemKNNCFRecommender(train)
        fit = _timed(lambda: model.fit(**p), reps)
        ev = EvaluatorHoldoutFast(test, [5, 10, 20])
        ev_full = EvaluatorHoldoutFast(test, [5, 10, 20], full_metrics=True)
        evaluate = _timed(lambda: ev.evaluateRecommender(model), reps)
        evaluate_full = _timed(lambda: ev_full.evaluateRecommender(model), reps)
        results, _ = ev.evaluateRecommender(model)
        # launches by class: one profiled fit and one profiled evaluation, runs of their own
        model.fit(**p)
        model.engine.profile(True)
        nnz = model.engine.itemknn_fit(0, min(p["topK"], model.n_items), shrink=float(p["shrink"]),
                                       den_a=np.sqrt(np.asarray(train.power(2).sum(axis=0)).ravel()),
                                       den_b=np.sqrt(np.asarray(train.power(2).sum(axis=0)).ravel()))
        fit_classes = model.engine.profile_read()
        model.engine.profile(True)
        ev.evaluateRecommender(model)
        eval_classes = model.engine.profile_read()
        model.engine.profile(False)
        row = dict(dataset=name, users=train.shape[0], items=train.shape[1], nnz=int(train.nnz), params=p, w_nnz=int(nnz),
                   evaluated_users=len(ev.usersToEvaluate), fit=fit, evaluate=evaluate, evaluate_full=evaluate_full,
                   fit_device_ms=float(sum(c["ms"] for c in fit_classes)), fit_classes=fit_classes, evaluate_classes=eval_classes,
                   MAP_at_5=float(results[5]["MAP"]))
        rows.append(row)
        print("%-10s %5d x %5d nnz %7d topK %4d: fit %.1f ms (device %.1f ms), evaluate %.1f ms, full row %.1f ms, MAP@5 %.6f" % (
            name, train.shape[0], train.shape[1], train.nnz, p["topK"], fit["median_ms"], row["fit_device_ms"],
            evaluate["median_ms"], evaluate_full["median_ms"], row["MAP_at_5"]), flush=True)
        for c in fit_classes + eval_classes:
            print("    %-44s %4d launches %9.3f ms" % (c["name"], c["launches"], c["ms"]))
        model.engine.close()
    return rows


def reference_bench(reference, reps):
    """the reference's own Python similarity on the CPU, same matrices and parameters (its Cython extension is not built)"""
    sys.path.insert(0, os.path.abspath(reference))
    for alias, kind in (("int", int), ("float", float), ("bool", bool), ("object", object)):
        if not hasattr(np, alias):      # aliases the reference still uses, removed in numpy 1.24
            setattr(np, alias, kind)
    from Base.Similarity.Compute_Similarity_Python import Compute_Similarity_Python
    params = json.load(open(os.path.join(GOLDEN, "itemknn_best_params_cosine.json")))
    rows = []
    for name, (train_file, _) in DATASETS.items():
        train = sps.load_npz(os.path.join(GOLDEN, train_file)).tocsr()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            Compute_Similarity_Python(train, **params[name]).compute_similarity()
            ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(dataset=name, reference_python_fit=_stats(ms)))
        print("%-10s reference Python fit on the CPU: median %.0f ms (min %.0f, max %.0f, %d reps)" % (
            name, np.median(ms), min(ms), max(ms), reps), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None, help="path of the reference tree: time its Python similarity on the CPU instead")
    a = ap.parse_args()
    rows = reference_bench(a.reference, a.reps) if a.reference else device_bench(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
