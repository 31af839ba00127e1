#!/usr/bin/env python3
"""Times the NMF solvers (ganmf_nmf_mu / ganmf_nmf_cd) with hipEvents on the library's stream, split by kernel class, and a whole
NMFRecommender.fit() with the wall clock.

  python tools/nmf_bench.py [--factors 100 25] [--iters 10] [--repeats 3] [--no-fit] [--sklearn]

One matrix: synthetic_urm(6040, 3706, density=0.045) (the ML-1M shape).  Per rank and solver (mu frobenius, mu kullback-leibler, cd)
it prints one JSON line with
  iter_ms         milliseconds per iteration: the stream timer around ONE call of --iters iterations (no error asked for)
  iter_ms_calls   the same iterations as one call each -- for cd the difference is the cost of the host read per iteration
  error_ms        one call of ganmf_nmf_error: what a check after every tenth iteration of the multiplicative update adds
  classes         per kernel class the launches and milliseconds of the --iters iterations with profiling on
  spmm            the sparse products against their gather bound: 4 k bytes per stored entry (+ the CSR arrays and the panel written)
  fit_s, n_iter_, transform_n_iter_    NMFRecommender.fit(num_factors=k, solver, beta_loss) after np.random.seed(0), wall clock
  sklearn_fit_s   with --sklearn: the reference's own call on this machine's CPU (context only)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVERS = [("mu", "frobenius"), ("mu", "kullback-leibler"), ("cd", "frobenius")]
NAMES = {"mu": "multiplicative_update", "cd": "coordinate_descent"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, nargs="+", default=[100, 25])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    from ganmf_amd import _lib as L
    from ganmf_amd.NMF import NMFRecommender, random_init
    from ganmf_amd.engine import Engine
    from ganmf_amd.synthetic import synthetic_urm
    shape = (6040, 3706)
    urm = sps.csr_matrix(synthetic_urm(shape[0], shape[1], density=0.045), dtype=np.float32)
    urm_t = sps.csr_matrix(urm.T)
    n = args.iters
    for k in args.factors:
        np.random.seed(k)
        W0, H0 = random_init(urm, k)
        rng = np.random.RandomState(k)
        perms = np.array([[rng.permutation(k), rng.permutation(k)] for _ in range(n)])
        for solver, loss in SOLVERS:
            beta = NMFRecommender.BETA_LOSS_CODES[loss]
            eng = Engine(shape[0], shape[1], k, 1, 1, model=L.MODEL_MF)
            eng.set_confidence(0, urm)
            eng.set_confidence(1, urm_t)

            def reset():
                eng.set_tensor(L.T_USER_EMB, W0)
                eng.set_tensor(L.T_ITEM_EMB, np.ascontiguousarray(H0.T))

            def run(calls):
                reset()
                eng.timer_start()
                for c in range(calls):
                    pm = perms[c * (n // calls):(c + 1) * (n // calls)]
                    if solver == "cd":
                        eng.nmf_cd(pm)
                    else:
                        eng.nmf_mu(beta, n // calls, True, error=False)
                return eng.timer_stop()

            run(1)                                   # warm-up: allocations, code objects
            one = [run(1) for _ in range(args.repeats)]
            many = [run(n) for _ in range(args.repeats)]
            eng.timer_start()
            eng.nmf_error(beta)
            error_ms = eng.timer_stop()
            eng.profile(True)
            run(1)
            classes = {c["name"]: {"launches": c["launches"], "ms": c["ms"]} for c in eng.profile_read()
                       if c["launches"] and "nmf" in c["name"]}
            eng.profile(False)
            eng.close()
            spmm = classes.get("nmf_spmm[rows,nnz]x[cols,k]", {"launches": 0, "ms": 0.0})
            spmm_bytes = spmm["launches"] * (4.0 * urm.nnz * k + 8.0 * urm.nnz) + 4.0 * k * (spmm["launches"] // 2) * (shape[0] + shape[1])
            row = {"shape": list(shape), "nnz": int(urm.nnz), "num_factors": k, "solver": solver, "beta_loss": loss, "iters": n,
                   "iter_ms": float(np.median(one)) / n, "iter_ms_calls": float(np.median(many)) / n, "error_ms": error_ms,
                   "classes": classes, "classes_ms_sum": float(sum(v["ms"] for v in classes.values())),
                   "spmm": {"launches": spmm["launches"], "gather_gbytes": spmm_bytes * 1e-9,
                            "gbytes_per_s": spmm_bytes / (spmm["ms"] * 1e-3) * 1e-9 if spmm["ms"] else None}}
            if not args.no_fit:
                model = NMFRecommender(urm)
                np.random.seed(0)
                t0 = time.time()
                model.fit(num_factors=k, solver=NAMES[solver], beta_loss=loss)
                row.update(fit_s=time.time() - t0, n_iter_=model.n_iter_, transform_n_iter_=model.transform_n_iter_,
                           reconstruction_err_=model.reconstruction_err_)
                model.engine.close()
            if args.sklearn:
                from sklearn.decomposition import NMF
                np.random.seed(0)
                t0 = time.time()
                m = NMF(n_components=k, init="random", solver=solver, beta_loss=loss, random_state=None, l1_ratio=0.5, shuffle=True,
                        max_iter=500)
                m.fit(urm)
                m.transform(urm)
                row.update(sklearn_fit_s=time.time() - t0, sklearn_n_iter_=m.n_iter_, sklearn_threads=os.environ.get("OMP_NUM_THREADS", ""))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
