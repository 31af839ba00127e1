#!/usr/bin/env python3
"""Writes tests/golden/nmf_tiny.npz: what sklearn.decomposition.NMF itself computes, in float32, on a few tiny matrices -- the
yardstick of tests/test_nmf_host.py (the float64 restatement of tests/helpers_nmf.py against it) and of tests/test_gpu_nmf.py (the
nndsvda start and the end-to-end records).  Needs scikit-learn; no test imports it.  Run from the repository root:

    python tools/make_nmf_fixture.py

Per case c (matrix [n_users, n_items], k factors, seed s; random_state=None throughout, so np.random.seed(s) governs every draw):
  c/X_data, X_indices, X_indptr, shape, k, seed
  c/random_W0, random_H0         _initialize_nmf(init="random") after np.random.seed(s)
  c/svd_U, svd_S, svd_V          randomized_svd(X, k) after np.random.seed(s): what init="nndsvda" starts from
  c/nndsvda_W0, nndsvda_H0       _initialize_nmf(init="nndsvda") after np.random.seed(s)
  c/perms                        [50, 2, k]: the permutations coordinate descent draws after np.random.seed(s) (W half, H half, ...)
  c/perms_t                      [50, k]: the ones transform() draws after np.random.seed(s)
  c/<solver>_<n>_W, _H, _err     W, components_ and reconstruction_err_ after n = 1 / 10 / 50 iterations at tol = 0 from random_W0 /
                                 random_H0, solver in mu_fro, mu_kl, cd
  c/<solver>_<n>_Wt              transform(X) of that model after n iterations at tol = 0 (W from sklearn's own start, H fixed)
End-to-end records of the LAST case, NMF(k, init, solver, beta_loss, random_state=None, l1_ratio=0.5, shuffle=True, max_iter=500)
.fit(X) then .transform(X) after np.random.seed(seed), seeds 0 .. 4:
  e2e/configs                    the (solver, beta_loss, init) names, "|"-joined
  e2e/n_iter, e2e/err            [configs, 5]: n_iter_ and reconstruction_err_"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import helpers_nmf as HN      # noqa: E402

# The seeds are chosen so that no entry of sqrt(S_j) u_j, sqrt(S_j) v_j of a non-empty row / column lies within 2e-4 of zero (float64 dense
# SVD) and the k leading singular values are at least 5e-3 sigma_1 apart: float32's rounding of the SVD (eps32 / gap, about 2e-5) then
# moves no entry across the 1e-6 threshold of init="nndsvda", in sklearn or on the device.  Among such seeds these are two where sklearn's
# own float32 SVD also leaves the row without an entry below the threshold (its U has rounding noise of 3e-7 there, which scaled by
# sqrt(S_j sigma) can pass 1e-6; the exact value, and the device's, is 0).
CASES = [("a", 40, 30, 4, 4), ("b", 130, 70, 9, 30)]
ITERS = (1, 10, 50)
SOLVERS = {"mu_fro": ("mu", "frobenius"), "mu_kl": ("mu", "kullback-leibler"), "cd": ("cd", "frobenius")}
E2E = [("mu", "frobenius", "random"), ("mu", "kullback-leibler", "random"), ("cd", "frobenius", "random"),
       ("mu", "frobenius", "nndsvda"), ("cd", "frobenius", "nndsvda")]
E2E_SEEDS = 5


def main():
    from sklearn.decomposition import NMF
    from sklearn.decomposition._nmf import _initialize_nmf
    from sklearn.utils.extmath import randomized_svd
    warnings.simplefilter("ignore")
    out = {}
    for name, n_users, n_items, k, seed in CASES:
        X = HN.case_matrix(n_users, n_items, seed)
        assert X.dtype == np.float32
        pre = name + "/"
        out[pre + "X_data"], out[pre + "X_indices"], out[pre + "X_indptr"] = X.data, X.indices, X.indptr
        out[pre + "shape"], out[pre + "k"], out[pre + "seed"] = np.array(X.shape), np.array(k), np.array(seed)
        np.random.seed(seed)
        W0, H0 = _initialize_nmf(X, k, init="random", random_state=None)
        out[pre + "random_W0"], out[pre + "random_H0"] = W0, H0
        np.random.seed(seed)
        U, S, V = randomized_svd(X, k, random_state=None)
        out[pre + "svd_U"], out[pre + "svd_S"], out[pre + "svd_V"] = U, S, V
        np.random.seed(seed)
        Wn, Hn = _initialize_nmf(X, k, init="nndsvda", random_state=None)
        out[pre + "nndsvda_W0"], out[pre + "nndsvda_H0"] = Wn, Hn
        np.random.seed(seed)
        out[pre + "perms"] = np.array([[np.random.permutation(k), np.random.permutation(k)] for _ in range(max(ITERS))])
        np.random.seed(seed)
        out[pre + "perms_t"] = np.array([np.random.permutation(k) for _ in range(max(ITERS))])
        for tag, (solver, loss) in SOLVERS.items():
            for n in ITERS:
                model = NMF(n_components=k, init="custom", solver=solver, beta_loss=loss, tol=0.0, max_iter=n, shuffle=True,
                            random_state=None)
                np.random.seed(seed)
                W = model.fit_transform(X, W=W0.copy(), H=H0.copy())
                assert model.n_iter_ == n and W.dtype == np.float32
                key = "%s%s_%d_" % (pre, tag, n)
                out[key + "W"], out[key + "H"], out[key + "err"] = W, model.components_.copy(), np.array(model.reconstruction_err_)
                np.random.seed(seed)
                out[key + "Wt"] = model.transform(X)
    # end to end at the reference's settings, on the last case
    n_it, errs = [], []
    for solver, loss, init in E2E:
        n_it.append([])
        errs.append([])
        for s in range(E2E_SEEDS):
            np.random.seed(s)
            model = NMF(n_components=k, init=init, solver=solver, beta_loss=loss, random_state=None, l1_ratio=0.5, shuffle=True,
                        max_iter=500)
            model.fit(X)
            model.transform(X)
            n_it[-1].append(model.n_iter_)
            errs[-1].append(model.reconstruction_err_)
    out["e2e/configs"] = np.array(["|".join(c) for c in E2E])
    out["e2e/n_iter"], out["e2e/err"] = np.array(n_it), np.array(errs)
    path = os.path.join(ROOT, "tests", "golden", "nmf_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print("e2e n_iter", out["e2e/n_iter"].tolist())
    print("e2e err", np.round(out["e2e/err"], 4).tolist())


if __name__ == "__main__":
    main()
