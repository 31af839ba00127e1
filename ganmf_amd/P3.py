"""P3alphaRecommender and RP3betaRecommender -- the graph-based item models, host mirrors of the reference classes
(GraphBased/P3alphaRecommender.py:19-141, GraphBased/RP3betaRecommender.py:16-151; the P3Alpha row of the comparison table in
RecSysExp.py:71-97).

Same constructors, fit() keyword arguments, W_sparse layout and saved-model layout as the reference, so they can stand in for
`GraphBased.P3alphaRecommender.P3alphaRecommender` and `GraphBased.RP3betaRecommender.RP3betaRecommender`.  The matrix -- a three-step
random walk item -> user -> item, Piu^alpha . Pui^alpha, its top-K per row, the optional row normalisation and the top-K per column
-- is computed by libganmf_hip.so (ganmf_p3_fit: HIP kernels on gfx950, on a GANMF_MODEL_ITEMSIM handle) and stays on the device,
where scoring -- URM_train[users] . W_sparse as a sparse product -- recommendation and evaluation run through the routes of
DeviceScoringMixin.  This file holds what the reference decides on the host: the min_rating / implicit filter of URM_train, and the
transition weights (the L1-normalised rows, the item degrees and their powers), formed in float64 and rounded to float32 once."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .similarity_model import SimilarityModelMixin


def transition_terms(URM_train, alpha, beta=None):
    """(row_scale, pui_by_item, col_scale) of one fit, float32:
    row_scale[i] = (1 / deg_i)^alpha, the one value of row i of Piu^alpha (0 for an item nobody rated);
    pui_by_item: items x users CSR in canonical form, the pattern of URM_train by item with the values (x_ui / sum_j |x_uj|)^alpha;
    col_scale[j] = deg_j^-beta (0 where deg_j = 0), None when beta is None.
    deg counts STORED entries: an explicit zero counts (the reference sets ones at every stored entry of the transpose)."""
    urm = SimilarityModelMixin._canonical(URM_train)
    n_users, n_items = urm.shape
    lengths = np.diff(urm.indptr)
    x = urm.data.astype(np.float64)
    l1 = np.bincount(np.repeat(np.arange(n_users), lengths), weights=np.abs(x), minlength=n_users)
    l1[l1 == 0.0] = 1.0      # (a row of stored zeros stays a row of zeros)
    p = x / np.repeat(l1, lengths)
    deg = np.bincount(urm.indices, minlength=n_items).astype(np.float64)
    some = deg > 0
    row_scale = np.zeros(n_items, dtype=np.float64)
    row_scale[some] = 1.0 / deg[some]
    if alpha != 1.0:
        p = np.power(p, float(alpha))
        row_scale[some] = np.power(row_scale[some], float(alpha))
    col_scale = None
    if beta is not None:
        col_scale = np.zeros(n_items, dtype=np.float64)
        col_scale[some] = np.power(deg[some], -float(beta))
        col_scale = col_scale.astype(np.float32)
    pui_by_item = SimilarityModelMixin._urm_by_item(sps.csr_matrix((p.astype(np.float32), urm.indices, urm.indptr), shape=urm.shape))
    return row_scale.astype(np.float32), pui_by_item, col_scale


class _GraphWalkRecommender(SimilarityModelMixin, DeviceScoringMixin, BaseRecommender):
    """what P3alpha and RP3beta share: everything but the popularity penalty"""

    MAX_TOPK = L.ITEMKNN_MAX_TOPK

    # what the device-scoring surface reads: as ItemKNNCFRecommender
    mode = "user"
    score_contract = "mf"
    mask_cold_users = False

    def __init__(self, URM_train, device=0, verbose=False):
        super(_GraphWalkRecommender, self).__init__(URM_train)
        self._URM_eval = self.URM_train
        self.device = device
        self.verbose = verbose
        self.engine = None

    def _fit_walk(self, topK, alpha, beta, min_rating, implicit, normalize_similarity):
        name = self.RECOMMENDER_NAME
        if int(topK) < 1:
            raise ValueError("{}: topK must be >= 1, provided was {}".format(name, topK))
        if not np.isfinite(alpha) or not alpha > 0:
            raise ValueError("{}: alpha must be finite and > 0, provided was {}".format(name, alpha))
        if beta is not None and not np.isfinite(beta):
            raise ValueError("{}: beta must be finite, provided was {}".format(name, beta))
        data = self.URM_train.data
        if data.size and (not np.all(np.isfinite(data)) or data.min() < 0):
            raise ValueError("{}: URM_train holds negative or non-finite ratings".format(name))
        topk = min(int(topK), self.n_items)      # (Recommender_utils.py:68; a row has no more than n_items entries either)
        if topk > self.MAX_TOPK:
            raise ValueError("{}: topK must be at most {} (the device selection runs topK rounds per item), provided was {}".format(
                name, self.MAX_TOPK, topK))
        self.topK = topK
        self.alpha = alpha
        self.min_rating = min_rating
        self.implicit = implicit
        self.normalize_similarity = normalize_similarity

        # as in the reference, URM_train is modified IN PLACE and the scores are formed from the modified matrix; `implicit` without
        # min_rating > 0 does nothing (P3alphaRecommender.py:46-50)
        if self.min_rating > 0:
            self.URM_train.data[self.URM_train.data < self.min_rating] = 0
            self.URM_train.eliminate_zeros()
            if self.implicit:
                self.URM_train.data = np.ones(self.URM_train.data.size, dtype=np.float32)
        self._URM_eval = self.URM_train

        self._build()      # the engine with URM_train (both orientations) and the seen mask
        row_scale, pui_by_item, col_scale = transition_terms(self.URM_train, alpha, beta)
        self.engine.set_confidence(1, pui_by_item)      # the walk reads the transition weights where the URM by item was
        self.engine.p3_fit(topk, row_scale, col_scale=col_scale, normalize=bool(normalize_similarity), col_topk=topk)
        self._restore_side1()


class P3alphaRecommender(_GraphWalkRecommender):
    """ P3alpha recommender """

    RECOMMENDER_NAME = "P3alphaRecommender"

    def __init__(self, URM_train, device=0, verbose=False):
        super(P3alphaRecommender, self).__init__(URM_train, device=device, verbose=verbose)

    def __str__(self):
        return "P3alpha(alpha={}, min_rating={}, topk={}, implicit={}, normalize_similarity={})".format(
            self.alpha, self.min_rating, self.topK, self.implicit, self.normalize_similarity)

    def fit(self, topK=100, alpha=1., min_rating=0, implicit=False, normalize_similarity=False):
        self._fit_walk(topK, alpha, None, min_rating, implicit, normalize_similarity)


class RP3betaRecommender(_GraphWalkRecommender):
    """ RP3beta recommender """

    RECOMMENDER_NAME = "RP3betaRecommender"

    def __init__(self, URM_train, device=0, verbose=False):
        super(RP3betaRecommender, self).__init__(URM_train, device=device, verbose=verbose)

    def __str__(self):
        return "RP3beta(alpha={}, beta={}, min_rating={}, topk={}, implicit={}, normalize_similarity={})".format(
            self.alpha, self.beta, self.min_rating, self.topK, self.implicit, self.normalize_similarity)

    def fit(self, alpha=1., beta=0.6, min_rating=0, topK=100, implicit=False, normalize_similarity=True):
        self._fit_walk(topK, alpha, float(beta), min_rating, implicit, normalize_similarity)
        self.beta = beta
