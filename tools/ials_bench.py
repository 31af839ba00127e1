#!/usr/bin/env python3
"""Times one epoch of implicit ALS (two calls of ganmf_als_half_sweep) at the ML-1M shape with hipEvents on the library's stream
and prints the algorithmic FLOPs and bytes beside it.

  python tools/ials_bench.py [--factors 25 250] [--epochs 5] [--helper]

Per rank it reports, per half sweep and per epoch, the milliseconds of the full profile matrix and of the same matrix with every row
cut to its FIRST entry: the second run keeps the Gram product and one factorisation and solve per warm row and removes the gather
and the rank update, so the two together say what bounds the kernel.  --helper also times the float32 numpy restatement
(tests/helpers_ials.py) for one epoch on the threads numpy is given (OMP_NUM_THREADS)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def first_entries(C):
    """the CSR matrix with only the first stored entry of every non-empty row"""
    C = sps.csr_matrix(C)
    n = np.ediff1d(C.indptr)
    keep = C.indptr[:-1][n > 0]
    indptr = np.concatenate([[0], np.cumsum(n > 0)]).astype(np.int64)
    return sps.csr_matrix((C.data[keep], C.indices[keep], indptr), shape=C.shape)


def algorithmic(C, k):
    """(FLOPs, bytes) of one epoch: two Gram products, per stored entry and side a symmetric rank-1 update and its share of b, per
    warm row one Cholesky factorisation and two substitutions; bytes: the gathered factor rows, the factors read and written"""
    U, N = C.shape
    nnz = C.nnz
    warm = int((np.ediff1d(C.indptr) > 0).sum() + (np.ediff1d(C.tocsc().indptr) > 0).sum())
    flops = 2.0 * (U + N) * k * k + 2 * nnz * (k * (k + 1) + 2.0 * k) + warm * (k ** 3 / 3.0 + 2.0 * k * k)
    nbytes = 4.0 * (2 * nnz * k + 2 * (U + N) * k + warm * k) + 2 * nnz * 8.0
    return flops, nbytes


def time_epochs(eng, epochs, reg, U0, V0):
    """mean milliseconds of (user half sweep, item half sweep) over `epochs` epochs behind one warm-up epoch.  Every timed call starts
    from the same full-rank random factors (uploaded outside the timed region): the time does not depend on the values, and the
    one-entry matrix would otherwise drive the factors to a rank far below k, where reg no longer covers the rounding of Y^T Y."""
    from ganmf_amd import _lib as L
    ms = np.zeros(2)
    for epoch in range(epochs + 1):
        for side in (0, 1):
            eng.set_tensor(L.T_USER_EMB, U0)
            eng.set_tensor(L.T_ITEM_EMB, V0)
            eng.timer_start()
            eng.als_half_sweep(side, reg)
            t = eng.timer_stop()
            if epoch > 0:
                ms[side] += t
    return ms / epochs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, nargs="+", default=[25, 250])
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--reg", type=float, default=1e-3)
    ap.add_argument("--alpha", type=float, default=3.0)
    ap.add_argument("--urm", default=os.path.join(ROOT, "tests", "golden", "Movielens1M_URM_train.npz"))
    ap.add_argument("--helper", action="store_true", help="also time one epoch of the float32 numpy restatement")
    args = ap.parse_args()
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = sps.load_npz(args.urm).tocsr().astype(np.float32)
    C = sps.csr_matrix(urm, copy=True)
    C.data = (1.0 + args.alpha * C.data).astype(np.float32)
    Ct = C.T.tocsr()
    out = []
    for k in args.factors:
        row = {"num_factors": k, "shape": list(urm.shape), "nnz": int(urm.nnz)}
        rng = np.random.RandomState(0)
        V0 = (k ** -0.5 * rng.random_sample((urm.shape[1], k))).astype(np.float32)
        U0 = (k ** -0.5 * rng.random_sample((urm.shape[0], k))).astype(np.float32)
        for label, c0, c1 in (("full", C, Ct), ("one_entry_per_row", first_entries(C), first_entries(Ct))):
            eng = Engine(urm.shape[0], urm.shape[1], k, 1, 1, model=L.MODEL_MF)
            eng.set_confidence(0, c0)
            eng.set_confidence(1, c1)
            ms = time_epochs(eng, args.epochs, args.reg, U0, V0)
            eng.close()
            row[label] = {"user_half_ms": float(ms[0]), "item_half_ms": float(ms[1]), "epoch_ms": float(ms.sum())}
        flops, nbytes = algorithmic(C, k)
        sec = row["full"]["epoch_ms"] * 1e-3
        row.update(algorithmic_gflop=flops * 1e-9, algorithmic_gbytes=nbytes * 1e-9, tflops=flops / sec * 1e-12, gbytes_per_s=nbytes / sec * 1e-9)
        if args.helper:
            from tests import helpers_ials as H
            U = np.zeros((urm.shape[0], k), np.float32)
            t0 = time.time()
            U = H.half_sweep(U, V0, C, args.reg, np.float32)
            H.half_sweep(V0, U, Ct, args.reg, np.float32)
            row["helper_float32_epoch_s"] = time.time() - t0
            row["helper_threads"] = os.environ.get("OMP_NUM_THREADS", "")
        out.append(row)
        print(json.dumps(row))
    return out


if __name__ == "__main__":
    main()
