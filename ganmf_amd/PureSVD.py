"""PureSVDRecommender -- truncated SVD of URM_train, host mirror of the reference class
(MatrixFactorization/PureSVDRecommender.py:15-43; "PureSVD" in the learned-MF studies of MFLearned.py).

Same constructor and fit() signature as the reference, so it can stand in for
`MatrixFactorization.PureSVDRecommender.PureSVDRecommender`.  The reference calls sklearn.utils.extmath.randomized_svd(URM_train,
n_components=num_factors, random_state=None) on the host; here the factorisation is one call of ganmf_pure_svd (sparse x dense
products, Cholesky-QR, a Jacobi eigensolver: HIP kernels on gfx950) on a GANMF_MODEL_MF handle.  This file holds what sklearn decides
on the host -- the number of random vectors, the number of power iterations, the orientation -- and the draw of the random test
matrix from numpy's GLOBAL stream, which is where random_state=None takes it from: after np.random.seed(s) the factors equal the
reference's up to float32.  Scoring, recommendation and evaluation are the device routes of DeviceScoringMixin under the MF
contract; the engine plumbing, the factor properties and persistence are FactorModelMixin's."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .factor_model import FactorModelMixin


def svd_plan(n_users, n_items, num_factors):
    """(n_random, n_iter, transposed) as randomized_svd chooses them with its defaults: n_oversamples = 10, n_iter = "auto" (7 when
    n_components < 0.1 min(shape), else 4), transpose = "auto" (the matrix is transposed when it has fewer rows than columns)"""
    k = int(num_factors)
    return k + 10, (7 if k < 0.1 * min(n_users, n_items) else 4), n_users < n_items


class PureSVDRecommender(FactorModelMixin, DeviceScoringMixin, BaseRecommender):
    RECOMMENDER_NAME = "PureSVDRecommender"

    OVERSAMPLES = 10
    MAX_FACTORS = L.SVD_MAX_RANDOM - OVERSAMPLES
    MAX_FACTORS_REASON = "fit() draws num_factors + {} random vectors, and ganmf_pure_svd takes at most {}".format(OVERSAMPLES, L.SVD_MAX_RANDOM)
    LOAD_CHECKS_MAX_FACTORS = False      # the limit is the factorisation's: factors of any width load and score

    mode = "user"
    score_contract = "mf"

    def __init__(self, URM_train, device=0, verbose=False):
        super(PureSVDRecommender, self).__init__(URM_train)
        self._URM_eval = self.URM_train
        self.device = device
        self.verbose = verbose
        self.use_bias = False
        self.engine = None
        self.num_factors = None
        self.Sigma = None

    def fit(self, num_factors=100):
        """The reference's fit().  Sigma (float32, [num_factors]) keeps the singular values, which the reference drops."""
        n_random, n_iter, transposed = svd_plan(self.n_users, self.n_items, num_factors)
        if int(num_factors) < 1:
            raise ValueError("{}: num_factors must be at least 1, provided was {}".format(self.RECOMMENDER_NAME, num_factors))
        if n_random > min(self.n_users, self.n_items):
            raise ValueError("{}: num_factors + {} = {} random vectors are more than min(n_users, n_items) = {}".format(
                self.RECOMMENDER_NAME, self.OVERSAMPLES, n_random, min(self.n_users, self.n_items)))
        if n_random > L.SVD_MAX_RANDOM:
            raise ValueError("{}: num_factors + {} = {} random vectors are above the device's limit of {} (SVD_MAX_RANDOM), provided "
                             "was num_factors = {}".format(self.RECOMMENDER_NAME, self.OVERSAMPLES, n_random, L.SVD_MAX_RANDOM, num_factors))
        self._build(num_factors)
        omega = np.random.normal(size=(min(self.n_users, self.n_items), n_random))
        urm = sps.csr_matrix(self.URM_train, dtype=np.float32)
        urm_t = urm.tocsc()
        self.engine.set_confidence(0, urm)
        self.engine.set_confidence(1, sps.csr_matrix((urm_t.data, urm_t.indices, urm_t.indptr), shape=(self.n_items, self.n_users)))
        if self.verbose:
            print("{}: {} random vectors, {} power iterations, {}".format(self.RECOMMENDER_NAME, n_random, n_iter,
                                                                           "URM^T" if transposed else "URM"))
        self.Sigma = self.engine.pure_svd(omega, n_iter)
        self._update_best_model()

    def _update_best_model(self):
        self.engine.snapshot_best()
