#!/usr/bin/env python3
"""First measurements of UserKNNCFRecommender on an MI355X, beside ItemKNNCFRecommender in the same process: fit(), the library call
of the fit with its kernels and its host part (the by-target result read back, turned into rows and uploaded inside
ganmf_userknn_fit), and a full hold-out evaluation, at the ML-1M shape -- the train / test fixtures of tests/golden/ or, when they are
absent, a synthetic matrix of the same shape and density.

  python tools/userknn_bench.py [--reps 7] [--out profile_out/userknn_bench.json]
  python tools/userknn_bench.py --reference /path/to/reference      # CPU only: the reference's Python class on the same fits

How the numbers are taken: every timed region is a host clock around a call that ends in a device synchronise (fit() and the library
call return after the last copy; evaluateRecommender returns metric values).  One untimed warm-up per region, then `reps`
repetitions; the median, the minimum and the maximum are reported.  The kernels are the profile classes of one further, profiled
call (hipEvent brackets, a run of its own); `host part of the call` is the median library call minus those kernels: the copies of
the counts and of the compact matrix, the counting sort on the host, the upload.  The transpose alone is also timed on the host, on
the matrix the call returned (`transpose_host`: the same counting sort, in scipy).  A run without a GPU fails: there is no fallback."""
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
SHAPE, NNZ, TEST_NNZ = (6040, 3706), 799983, 200226      # ML-1M's train / test split
PARAMS = [dict(topK=50, shrink=100, similarity="cosine", normalize=True),      # fit()'s defaults
          dict(topK=297, shrink=0, similarity="cosine", normalize=True)]       # ItemKNN's tuned ML-1M row


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


def _synthetic(nnz, seed):
    """ratings 1..5 at ML-1M's shape with popularity-skewed items and activity-skewed users"""
    rng = np.random.RandomState(seed)
    pu = rng.lognormal(0.0, 1.0, SHAPE[0])
    pi = rng.lognormal(0.0, 1.3, SHAPE[1])
    rows = rng.choice(SHAPE[0], size=2 * nnz, p=pu / pu.sum())
    cols = rng.choice(SHAPE[1], size=2 * nnz, p=pi / pi.sum())
    keep = np.unique(rows.astype(np.int64) * SHAPE[1] + cols)
    keep = rng.permutation(keep)[:nnz]
    return sps.csr_matrix((rng.randint(1, 6, len(keep)).astype(np.float32), (keep // SHAPE[1], keep % SHAPE[1])), shape=SHAPE)


def load():
    files = [os.path.join(GOLDEN, f) for f in ("Movielens1M_URM_train.npz", "Movielens1M_URM_test.npz")]
    if all(os.path.exists(f) for f in files):
        return "ML-1M fixtures", sps.load_npz(files[0]).tocsr(), sps.load_npz(files[1]).tocsr()
    return "synthetic, ML-1M's shape and density", _synthetic(NNZ, 1), _synthetic(TEST_NNZ, 2)


def _norms(train, axis):
    return np.sqrt(np.asarray(sps.csr_matrix(train, dtype=np.float64).power(2).sum(axis=axis)).ravel())


def device_bench(reps):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender
    from ganmf_amd.UserKNN import UserKNNCFRecommender
    source, train, test = load()
    ev = EvaluatorHoldoutFast(test, [5, 10, 20])
    ev_full = EvaluatorHoldoutFast(test, [5, 10, 20], full_metrics=True)
    rows = []
    for p in PARAMS:
        for cls, call, axis in ((UserKNNCFRecommender, "userknn_fit", 1), (ItemKNNCFRecommender, "itemknn_fit", 0)):
            model = cls(train)
            fit = _timed(lambda: model.fit(**p), reps)
            evaluate = _timed(lambda: ev.evaluateRecommender(model), reps)
            evaluate_full = _timed(lambda: ev_full.evaluateRecommender(model), reps)
            results, _ = ev.evaluateRecommender(model)
            eng, norm = model.engine, _norms(train, axis)
            k = min(p["topK"], train.shape[1 - axis])
            lib_call = lambda: getattr(eng, call)(0, k, shrink=float(p["shrink"]), den_a=norm, den_b=norm)
            call_ms = _timed(lib_call, reps)
            eng.profile(True)      # launches by class: one profiled call and one profiled evaluation, runs of their own
            nnz = lib_call()
            fit_classes = eng.profile_read()
            eng.profile(True)
            ev.evaluateRecommender(model)
            eval_classes = eng.profile_read()
            eng.profile(False)
            W = model.W_sparse
            kernels = float(sum(c["ms"] for c in fit_classes))
            row = dict(model=cls.RECOMMENDER_NAME, data=source, users=train.shape[0], items=train.shape[1], nnz=int(train.nnz), params=p,
                       w_nnz=int(nnz), longest_row=int(np.diff(W.indptr).max()), evaluated_users=len(ev.usersToEvaluate), fit=fit,
                       library_call=call_ms, fit_kernels_ms=kernels, call_host_part_ms=call_ms["median_ms"] - kernels,
                       evaluate=evaluate, evaluate_full=evaluate_full, fit_classes=fit_classes, evaluate_classes=eval_classes,
                       MAP_at_5=float(results[5]["MAP"]))
            if axis == 1:
                by_target = sps.csc_matrix(W)
                row["transpose_host"] = _timed(lambda: by_target.tocsr(), reps)
            rows.append(row)
            print("%-22s %s topK %3d shrink %3d: fit() %.1f ms, library call %.1f ms (kernels %.2f ms, host part %.1f ms%s), W nnz %d, "
                  "longest row %d, evaluate %.1f ms, full row %.1f ms, MAP@5 %.6f" % (
                      row["model"], source, p["topK"], p["shrink"], fit["median_ms"], call_ms["median_ms"], kernels, row["call_host_part_ms"],
                      ", scipy transpose alone %.1f ms" % row["transpose_host"]["median_ms"] if axis == 1 else "", nnz, row["longest_row"],
                      evaluate["median_ms"], evaluate_full["median_ms"], row["MAP_at_5"]), flush=True)
            for c in fit_classes + eval_classes:
                print("    %-44s %4d launches %9.3f ms" % (c["name"], c["launches"], c["ms"]))
            eng.close()
    return rows


def reference_bench(reference, reps):
    """the reference's own Python similarity of URM_train.T and its CSR conversion on the CPU (its Cython extension is not built)"""
    sys.path.insert(0, os.path.abspath(reference))
    for alias, kind in (("int", int), ("float", float), ("bool", bool), ("object", object)):
        if not hasattr(np, alias):      # aliases the reference still uses, removed in numpy 1.24
            setattr(np, alias, kind)
    from Base.Similarity.Compute_Similarity_Python import Compute_Similarity_Python
    source, train, _ = load()
    rows = []
    for p in PARAMS:
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            sps.csr_matrix(Compute_Similarity_Python(train.T, **p).compute_similarity())
            ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(data=source, params=p, reference_python_fit=_stats(ms)))
        print("topK %3d shrink %3d: reference Python user fit on the CPU: median %.0f ms (min %.0f, max %.0f, %d reps)" % (
            p["topK"], p["shrink"], np.median(ms), min(ms), max(ms), reps), flush=True)
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
