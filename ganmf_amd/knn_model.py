"""What the two collaborative neighbourhood models share on the host (ItemKNN.py, UserKNN.py; the reference's
KNN/ItemKNNCFRecommender.py:18-54 and KNN/UserKNNCFRecommender.py:18-61, which differ in one transpose): the feature weightings, fit()'s
arguments and their errors, which similarities binarise the data and switch `normalize` off, and the per-target terms of the
denominators (Base/Similarity/Compute_Similarity_Python.py:51-107, 233-250).  A subclass says which side of the URM holds its targets
(`_fit_side`: 1 the items, 0 the users) and which engine call fits (`_device_fit`)."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .similarity_model import SimilarityModelMixin


def okapi_BM_25(dataMatrix, K1=1.2, B=0.75):
    """Okapi BM25 weights of a sparse matrix whose rows are the documents (here: items) and columns the terms (users); float64 CSR.
    (Base/IR_feature_weighting.py:13-43)"""
    if not (0 < B < 1) or not K1 > 0:
        raise ValueError("okapi_BM_25: B must be in (0, 1) and K1 > 0")
    m = sps.coo_matrix(dataMatrix)
    n_docs = float(m.shape[0])
    idf = np.log(n_docs / (1 + np.bincount(m.col, minlength=m.shape[1])))
    doc_len = np.ravel(m.sum(axis=1))
    length_norm = (1.0 - B) + B * doc_len / doc_len.mean()
    data = m.data * (K1 + 1.0) / (K1 * length_norm[m.row] + m.data) * idf[m.col]
    return sps.coo_matrix((data, (m.row, m.col)), shape=m.shape).tocsr()


def TF_IDF(dataMatrix):
    """TF-IDF weights, rows = documents (items), columns = terms (users): sqrt(tf) * idf; float64 CSR.
    (Base/IR_feature_weighting.py:48-65)"""
    m = sps.coo_matrix(dataMatrix)
    n_docs = float(m.shape[0])
    idf = np.log(n_docs / (1 + np.bincount(m.col, minlength=m.shape[1])))
    data = np.sqrt(m.data) * idf[m.col]
    return sps.coo_matrix((data, (m.row, m.col)), shape=m.shape).tocsr()


class NeighbourhoodCFRecommender(SimilarityModelMixin, DeviceScoringMixin, BaseRecommender):
    FEATURE_WEIGHTING_VALUES = ["BM25", "TF-IDF", "none"]
    SIMILARITY_VALUES = ["cosine", "asymmetric", "jaccard", "tanimoto", "dice", "tversky"]
    # the reference's other modes change the data (mean removal, distances): not computed by this library
    SIMILARITY_NOT_BUILT = ["adjusted", "pearson", "euclidean"]
    MAX_TOPK = L.ITEMKNN_MAX_TOPK

    # what the device-scoring surface reads: users are rows; `items_to_compute` is honoured (Base/BaseSimilarityMatrixRecommender.py:
    # 85-88), but a user without interactions scores 0 everywhere instead of -inf: the item filter of the MF contract without its
    # cold-user mask
    mode = "user"
    score_contract = "mf"
    mask_cold_users = False

    _fit_side = 1      # the side of the handle whose rows are the targets of the similarity: 1 items x users, 0 users x items
    _target = "item"

    def __init__(self, URM_train, device=0, verbose=False):
        super(NeighbourhoodCFRecommender, self).__init__(URM_train)
        self._URM_eval = self.URM_train
        self.device = device
        self.verbose = verbose
        self.engine = None

    def _n_targets(self):
        return self.n_items if self._fit_side == 1 else self.n_users

    def _device_fit(self, kind, topk, **kw):
        raise NotImplementedError

    def _similarity_plan(self, similarity, normalize, shrink, asymmetric_alpha, tversky_alpha, tversky_beta):
        """(kind, binarise, p0, p1): which denominator the device applies (L.ITEMKNN_*), whether the data are replaced by ones, and
        the two Tversky coefficients (Compute_Similarity_Python.py:70-95, 309-336)"""
        if similarity in ("jaccard", "tanimoto"):
            return L.ITEMKNN_TANIMOTO, True, 1.0, 1.0
        if similarity == "dice":
            return L.ITEMKNN_DICE, True, 1.0, 1.0
        if similarity == "tversky":
            return L.ITEMKNN_TVERSKY, True, float(tversky_alpha), float(tversky_beta)
        if normalize:
            return L.ITEMKNN_PRODUCT, False, 1.0, 1.0
        return (L.ITEMKNN_SHRINK_ONLY if shrink != 0 else L.ITEMKNN_RAW), False, 1.0, 1.0

    def _set_fit_side(self, urm):
        """`urm` (users x items, canonical) to the side the fit reads; returns what was uploaded"""
        m = urm if self._fit_side == 0 else self._urm_by_item(urm)
        self.engine.set_confidence(self._fit_side, m)
        return m

    def fit(self, topK=50, shrink=100, similarity='cosine', normalize=True, feature_weighting="none", **similarity_args):
        """The reference's fit().  similarity_args: asymmetric_alpha (default 0.5), tversky_alpha, tversky_beta (default 1.0).  Not
        built, ValueError: the similarities 'adjusted', 'pearson' and 'euclidean', and row_weights."""
        if feature_weighting not in self.FEATURE_WEIGHTING_VALUES:
            raise ValueError("Value for 'feature_weighting' not recognized. Acceptable values are {}, provided was '{}'".format(
                self.FEATURE_WEIGHTING_VALUES, feature_weighting))
        if similarity in self.SIMILARITY_NOT_BUILT:
            raise ValueError("{}: similarity '{}' is not built by this implementation; available are {}".format(
                self.RECOMMENDER_NAME, similarity, self.SIMILARITY_VALUES))
        if similarity not in self.SIMILARITY_VALUES:
            raise ValueError("Cosine_Similarity: value for parameter 'mode' not recognized. Allowed values are: {}. Passed value was "
                             "'{}'".format(self.SIMILARITY_VALUES + self.SIMILARITY_NOT_BUILT, similarity))
        args = dict(asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0, row_weights=None)
        for name in similarity_args:
            if name not in args:
                raise TypeError("{}.fit() got an unexpected similarity argument '{}'".format(self.RECOMMENDER_NAME, name))
        args.update(similarity_args)
        if args["row_weights"] is not None:
            raise ValueError("{}: row_weights is not built by this implementation".format(self.RECOMMENDER_NAME))
        if int(topK) < 1:
            raise ValueError("{}: topK must be >= 1, provided was {}".format(self.RECOMMENDER_NAME, topK))
        if not shrink >= 0:
            raise ValueError("{}: shrink must be >= 0, provided was {}".format(self.RECOMMENDER_NAME, shrink))
        topk = min(int(topK), self._n_targets())      # (Compute_Similarity_Python.py:55)
        if topk > self.MAX_TOPK:
            raise ValueError("{}: topK must be at most {} (the device selection runs topK rounds per {}), provided was {}".format(
                self.RECOMMENDER_NAME, self.MAX_TOPK, self._target, topK))
        self.topK = topK
        self.shrink = shrink

        # as in the reference, the weighted matrix REPLACES URM_train: the scores are formed from it too
        if feature_weighting == "BM25":
            self.URM_train = sps.csr_matrix(okapi_BM_25(self.URM_train.astype(np.float32).T).T)
        elif feature_weighting == "TF-IDF":
            self.URM_train = sps.csr_matrix(TF_IDF(self.URM_train.astype(np.float32).T).T)
        self._URM_eval = self.URM_train

        kind, binarise, p0, p1 = self._similarity_plan(similarity, normalize, shrink, args["asymmetric_alpha"],
                                                       args["tversky_alpha"], args["tversky_beta"])
        self._build()      # the engine with URM_train (both orientations) and the seen mask
        den_a = den_b = None
        if binarise:
            # the similarity sees ones at the stored entries; the scores keep URM_train's values
            ones = self._canonical(self.URM_train)
            ones.data[:] = 1.0
            seen = self._set_fit_side(ones)
            den_a = np.diff(seen.indptr).astype(np.float64)      # sums of squares of a target's vector of ones
        elif kind == L.ITEMKNN_PRODUCT:
            # what the device multiplies, by target: the columns (items) or the rows (users)
            data32 = (sps.csc_matrix if self._fit_side == 1 else sps.csr_matrix)(self.URM_train, dtype=np.float32)
            sq = np.asarray(data32.astype(np.float64).power(2).sum(axis=0 if self._fit_side == 1 else 1)).ravel()
            norm = np.sqrt(sq)
            if similarity == "asymmetric":
                alpha = float(args["asymmetric_alpha"])
                den_a, den_b = np.power(norm, 2 * alpha), np.power(norm, 2 * (1 - alpha))
            else:
                den_a = den_b = norm
        self._device_fit(kind, topk, shrink=float(shrink), p0=p0, p1=p1, den_a=den_a, den_b=den_b)
        if binarise:
            self._set_fit_side(self._canonical(self.URM_train))      # back to URM_train's own values before anything is scored
