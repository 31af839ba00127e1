#!/usr/bin/env python3
"""Times one PureSVD factorisation (one call of ganmf_pure_svd) with hipEvents on the library's stream, split by kernel class, and
the sklearn call it replaces on the same box.

  python tools/puresvd_bench.py [--factors 10 50 250] [--repeats 3] [--no-sklearn]

Two matrices: synthetic_urm(6040, 3706, density=0.045) (the ML-1M shape) and synthetic_urm(1884, 17632, density=0.00223) (the small
LastFM-like shape, the transposed branch).  Per matrix and rank it prints one JSON line with
  fit_ms          the whole call: uploads of omega, every kernel, the flag read-back (stream timer around Engine.pure_svd)
  classes         per kernel class the launches and milliseconds of one call with profiling on (ganmf_profile_read): sparse
                  products, Gram products and apply products with their split-K sums, Cholesky + inverse, Jacobi, select / sign
  spmm            the bytes the sparse products' gather has to move (4 l per stored entry, the CSR arrays, the panel written) and
                  the achieved bytes/s
  sklearn_s       sklearn.utils.extmath.randomized_svd(URM, n_components=k, random_state=None) on the threads the machine grants
                  (OMP_NUM_THREADS)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASS_PREFIX = ("svd_", "reduce_svd_")


def plan(shape, k):
    return k + 10, (7 if k < 0.1 * min(shape) else 4)


def one_fit(eng, omega, n_iter):
    eng.timer_start()
    sigma = eng.pure_svd(omega, n_iter)
    return eng.timer_stop(), sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, nargs="+", default=[10, 50, 250])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    from ganmf_amd.synthetic import synthetic_urm
    out = []
    for name, shape, density in (("ml1m_shape", (6040, 3706), 0.045), ("lastfm_shape", (1884, 17632), 0.00223)):
        urm = synthetic_urm(shape[0], shape[1], density=density).astype(np.float32)
        urm_t = sps.csr_matrix(urm.T)
        for k in args.factors:
            l, n_iter = plan(shape, k)
            omega = np.random.RandomState(k).normal(size=(min(shape), l))
            eng = Engine(shape[0], shape[1], k, 1, 1, model=L.MODEL_MF)
            eng.set_confidence(0, urm)
            eng.set_confidence(1, urm_t)
            one_fit(eng, omega, n_iter)                                   # warm-up: allocations, code objects
            ms = [one_fit(eng, omega, n_iter)[0] for _ in range(args.repeats)]
            eng.profile(True)
            _, sigma = one_fit(eng, omega, n_iter)
            classes = {c["name"]: {"launches": c["launches"], "ms": c["ms"]} for c in eng.profile_read()
                       if c["launches"] and c["name"].startswith(CLASS_PREFIX)}
            eng.profile(False)
            eng.close()
            n_spmm = 2 * n_iter + 2
            spmm_bytes = n_spmm * (4.0 * urm.nnz * l + 8.0 * urm.nnz) + 4.0 * l * ((n_iter + 1) * shape[0] + (n_iter + 1) * shape[1])
            spmm_ms = sum(v["ms"] for n, v in classes.items() if n.startswith("svd_spmm"))
            row = {"matrix": name, "shape": list(shape), "nnz": int(urm.nnz), "num_factors": k, "n_random": l, "n_iter": n_iter,
                   "fit_ms": float(np.median(ms)), "fit_ms_all": [float(x) for x in ms], "classes": classes,
                   "classes_ms_sum": float(sum(v["ms"] for v in classes.values())),
                   "spmm": {"launches": n_spmm, "gather_gbytes": spmm_bytes * 1e-9,
                            "gbytes_per_s": spmm_bytes / (spmm_ms * 1e-3) * 1e-9 if spmm_ms else None},
                   "sigma_first_last": [float(sigma[0]), float(sigma[-1])]}
            if not args.no_sklearn:
                try:
                    from sklearn.utils.extmath import randomized_svd
                    t0 = time.time()
                    randomized_svd(sps.csr_matrix(urm, dtype=np.float64), n_components=k, random_state=None)
                    row["sklearn_s"] = time.time() - t0
                    row["sklearn_threads"] = os.environ.get("OMP_NUM_THREADS", "")
                except ImportError:
                    row["sklearn_s"] = None
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


if __name__ == "__main__":
    main()
