"""NMFRecommender -- non-negative matrix factorisation of URM_train, host mirror of the reference class
(MatrixFactorization/NMFRecommender.py:15-78).

Same constructor, fit() signature, class attributes, messages and coin flip as the reference, so it can stand in for
`MatrixFactorization.NMFRecommender.NMFRecommender`.  The reference fits sklearn.decomposition.NMF(n_components=num_factors, init,
solver, beta_loss, random_state=None, l1_ratio, shuffle=True, max_iter=500) on the host and then solves a second time, transform(),
for the user factors; both alphas keep their default 0, so no regularisation term exists and l1_ratio is validated and otherwise
unused.  Here the solvers run on the device (ganmf_nmf_mu / ganmf_nmf_cd / ganmf_nmf_error on a GANMF_MODEL_MF handle: HIP kernels on
gfx950, ganmf_amd/csrc/nmf_rows.hpp).  This file holds what sklearn decides on the host: the initial factors, every random number --
random_state=None is numpy's GLOBAL stream, so after np.random.seed(s) the draws are sklearn's, in sklearn's order, and the stream
is left where sklearn leaves it -- the two stopping rules (tol = 1e-4) and the order fit -> transform.  ITEM_factors is components_.T,
USER_factors is transform(URM_train): the second solve with H fixed, not the W of the fit.  n_iter_ and reconstruction_err_ are the
fit's, transform_n_iter_ the second solve's.  Scoring, recommendation and evaluation are the device routes of DeviceScoringMixin
under the MF contract; the engine plumbing, the factor properties and persistence are FactorModelMixin's."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .PureSVD import svd_plan
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .factor_model import FactorModelMixin

NNDSVD_EPS = 1e-6      # sklearn's _initialize_nmf(eps=1e-6): smaller entries of the split become 0


def random_init(urm, num_factors):
    """sklearn's init="random": (W [n_users, k], H [k, n_items]) = |avg * standard_normal|, H drawn FIRST, from numpy's global stream"""
    n_users, n_items = urm.shape
    avg = np.sqrt(urm.mean() / num_factors)
    H = avg * np.random.standard_normal(size=(num_factors, n_items)).astype(urm.dtype, copy=False)
    W = avg * np.random.standard_normal(size=(n_users, num_factors)).astype(urm.dtype, copy=False)
    return np.abs(W), np.abs(H)


def nndsvda_split(U, S, V, mean):
    """sklearn's init="nndsvda" from the truncated SVD U [n_users, k], S [k], V [k, n_items]: column 0 is sqrt(S0) |u0|, sqrt(S0) |v0|;
    column j >= 1 keeps the positive or the negative parts of (u_j, v_j), whichever pair has the larger product of norms (the
    positive one only if strictly larger), each unit vector scaled by sqrt(S_j * that product); entries below 1e-6 become 0 and every
    exact 0 becomes `mean`"""
    W, H = np.zeros_like(U), np.zeros_like(V)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(V[0, :])
    for j in range(1, U.shape[1]):
        x, y = U[:, j], V[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = np.sqrt(np.dot(x_p, x_p)), np.sqrt(np.dot(y_p, y_p))
        x_n_nrm, y_n_nrm = np.sqrt(np.dot(x_n, x_n)), np.sqrt(np.dot(y_n, y_n))
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        else:
            u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * u
        H[j, :] = lbd * v
    W[W < NNDSVD_EPS] = 0
    H[H < NNDSVD_EPS] = 0
    W[W == 0] = mean
    H[H == 0] = mean
    return W, H


class NMFRecommender(FactorModelMixin, DeviceScoringMixin, BaseRecommender):
    """ Non Negative Matrix Factorization Recommender

    https://scikit-learn.org/stable/modules/generated/sklearn.decomposition.NMF.html

    """

    RECOMMENDER_NAME = "NMFRecommender"

    SOLVER_VALUES = {"coordinate_descent": "cd",
                     "multiplicative_update": "mu"}

    INIT_VALUES = ["random", "nndsvda"]
    # random: non-negative random matrices, scaled with sqrt(X.mean() / n_components)
    # nndsvda: Nonnegative Double Singular Value Decomposition with zeros filled with the average of X

    BETA_LOSS_VALUES = ["frobenius", "kullback-leibler"]

    BETA_LOSS_CODES = {"frobenius": L.NMF_FROBENIUS, "kullback-leibler": L.NMF_KULLBACK_LEIBLER}
    MAX_ITER = 500           # the reference's max_iter
    TOL = 1e-4               # sklearn's default tol
    MU_CHECK_EVERY = 10      # the multiplicative update tests its criterion after every 10th iteration: one host read per chunk
    OVERSAMPLES = 10         # randomized_svd's n_oversamples, as init="nndsvda" calls it
    MAX_FACTORS = L.NMF_MAX_FACTORS
    MAX_FACTORS_REASON = ("the coordinate-descent kernel keeps a row of a factor in {} registers per lane of one wave, and "
                          "init='nndsvda' draws num_factors + {} random vectors of the {} ganmf_pure_svd takes").format(
                              (L.NMF_MAX_FACTORS + 63) // 64, OVERSAMPLES, L.SVD_MAX_RANDOM)
    LOAD_CHECKS_MAX_FACTORS = False      # the limit is the factorisation's: factors of any width load and score

    mode = "user"
    score_contract = "mf"

    def __init__(self, URM_train, device=0):
        super(NMFRecommender, self).__init__(URM_train)
        self._URM_eval = self.URM_train
        self.device = device
        self.use_bias = False
        self.engine = None
        self.num_factors = None
        self.n_iter_ = None
        self.reconstruction_err_ = None
        self.transform_n_iter_ = None

    def fit(self, num_factors=100,
            l1_ratio=0.5,
            solver="multiplicative_update",
            init_type="random",
            beta_loss="frobenius",
            verbose=False):

        assert l1_ratio >= 0 and l1_ratio <= 1, "{}: l1_ratio must be between 0 and 1, provided value was {}".format(self.RECOMMENDER_NAME, l1_ratio)

        if solver not in self.SOLVER_VALUES:
            raise ValueError("Value for 'solver' not recognized. Acceptable values are {}, provided was '{}'".format(self.SOLVER_VALUES.keys(), solver))

        if init_type not in self.INIT_VALUES:
            raise ValueError("Value for 'init_type' not recognized. Acceptable values are {}, provided was '{}'".format(self.INIT_VALUES, init_type))

        if beta_loss not in self.BETA_LOSS_VALUES:
            raise ValueError("Value for 'beta_loss' not recognized. Acceptable values are {}, provided was '{}'".format(self.BETA_LOSS_VALUES, beta_loss))

        if int(num_factors) < 1 or int(num_factors) > self.MAX_FACTORS:
            raise ValueError("{}: num_factors must be in [1, {}] ({}), provided was {}".format(
                self.RECOMMENDER_NAME, self.MAX_FACTORS, self.MAX_FACTORS_REASON, num_factors))
        k = int(num_factors)
        if init_type == "nndsvda":
            if k > min(self.n_users, self.n_items):
                raise ValueError("init = '{}' can only be used when n_components <= min(n_samples, n_features)".format(init_type))
            if k + self.OVERSAMPLES > min(self.n_users, self.n_items):
                raise ValueError("{}: init_type 'nndsvda' draws num_factors + {} = {} random vectors, more than min(n_users, n_items) "
                                 "= {}".format(self.RECOMMENDER_NAME, self.OVERSAMPLES, k + self.OVERSAMPLES, min(self.n_users, self.n_items)))

        if solver == 'coordinate_descent' and beta_loss == 'kullback-leibler':
            coin_flip = np.random.binomial(1, 0.5, 1)
            if coin_flip:
                solver = 'multiplicative_update'
            else:
                beta_loss = 'frobenius'

        self._build(k)
        urm = sps.csr_matrix(self.URM_train, dtype=np.float32)
        urm_t = urm.tocsc()
        self.engine.set_confidence(0, urm)
        self.engine.set_confidence(1, sps.csr_matrix((urm_t.data, urm_t.indices, urm_t.indptr), shape=(self.n_items, self.n_users)))

        W, H = self._initial_factors(urm, k, init_type)
        self.engine.set_tensor(L.T_USER_EMB, W)
        self.engine.set_tensor(L.T_ITEM_EMB, np.ascontiguousarray(H.T))
        mu, beta = self.SOLVER_VALUES[solver] == "mu", self.BETA_LOSS_CODES[beta_loss]
        if mu:
            self.n_iter_, err = self._run_mu(beta, True)
            # (the error of the last check is the final one only if the loop stopped there)
            self.reconstruction_err_ = err if err is not None else self.engine.nmf_error(beta)
        else:
            self.n_iter_ = self._run_cd(True)
            self.reconstruction_err_ = self.engine.nmf_error(beta)
        if verbose:
            print("{}: {} iterations of {}, {} loss: reconstruction error {:.6g}".format(
                self.RECOMMENDER_NAME, self.n_iter_, solver, beta_loss, self.reconstruction_err_))

        # USER_factors = transform(URM_train): H fixed, W from sklearn's start of that solve
        start = np.sqrt(urm.mean() / k) if mu else 0.0
        self.engine.set_tensor(L.T_USER_EMB, np.full((self.n_users, k), start, dtype=np.float32))
        self.transform_n_iter_ = self._run_mu(beta, False)[0] if mu else self._run_cd(False)
        if verbose:
            print("{}: transform: {} iterations".format(self.RECOMMENDER_NAME, self.transform_n_iter_))
        self._update_best_model()

    def _initial_factors(self, urm, k, init_type):
        """(W [n_users, k], H [k, n_items]) float32 as sklearn's _initialize_nmf draws them"""
        if init_type == "random":
            return random_init(urm, k)
        n_random, n_iter, _ = svd_plan(self.n_users, self.n_items, k)
        omega = np.random.normal(size=(min(self.n_users, self.n_items), n_random))
        S = self.engine.pure_svd(omega, n_iter)
        U = self.engine.get_tensor(L.T_USER_EMB)
        V = np.ascontiguousarray((self.engine.get_tensor(L.T_ITEM_EMB) / S).T)      # ITEM_factors = V^T diag(S)
        return nndsvda_split(U, S, V, urm.mean())

    def _run_mu(self, beta, update_H):
        """sklearn's _fit_multiplicative_update loop: (n_iter, the error if the loop stopped at a check, else None)"""
        error_at_init = self.engine.nmf_error(beta)
        previous = error_at_init
        done = 0
        while done < self.MAX_ITER:
            chunk = min(self.MU_CHECK_EVERY, self.MAX_ITER - done)
            check = chunk == self.MU_CHECK_EVERY
            err = self.engine.nmf_mu(beta, chunk, update_H, error=check)
            done += chunk
            if check:
                # a perfect start has error_at_init == 0: numpy's nan compares False and the loop carries on, as in sklearn
                with np.errstate(divide="ignore", invalid="ignore"):
                    stop = np.float64(previous - err) / np.float64(error_at_init) < self.TOL
                if stop:
                    return done, err
                previous = err
        return done, (err if check else None)

    def _run_cd(self, update_H):
        """sklearn's _fit_coordinate_descent loop: one permutation per half from the global stream, drawn only for the iterations that
        run; returns n_iter"""
        k, halves = self.num_factors, 2 if update_H else 1
        violation_init = None
        for n_iter in range(1, self.MAX_ITER + 1):
            perms = np.stack([np.random.permutation(k) for _ in range(halves)])
            violation = float(self.engine.nmf_cd(perms[None], update_H)[0])
            if n_iter == 1:
                violation_init = violation
            if violation_init == 0:
                break
            if violation / violation_init <= self.TOL:
                break
        return n_iter

    def _update_best_model(self):
        self.engine.snapshot_best()
