"""User-KNN in numpy float64: the reference's UserKNNCFRecommender computes the similarity of URM_train.T (KNN/UserKNNCFRecommender.py:
58), so the fit is helpers_itemknn's on the transposed matrix, under the same tie rule; the scores are W[users] . URM
(Base/BaseSimilarityMatrixRecommender.py:95-117).  Nothing here imports the reference."""
import numpy as np
import scipy.sparse as sps

from tests import helpers_itemknn as H

EPS32 = H.EPS32


def host_plan(urm, similarity, normalize, shrink, **kw):
    """helpers_itemknn.host_plan of the transposed matrix: (kind, X dense [items, users], p0, p1, den_a, den_b), the den per USER"""
    return H.host_plan(sps.csr_matrix(urm).T.tocsr(), similarity, normalize, shrink, **kw)


def fit(urm, topK=50, shrink=100, similarity="cosine", normalize=True, **kw):
    """W_sparse (CSR float64 [users, users]; column i = the kept neighbours of user i) of the reference's fit() without weighting"""
    return H.fit(sps.csr_matrix(urm).T.tocsr(), topK=topK, shrink=shrink, similarity=similarity, normalize=normalize, **kw)


def scores(urm, W, users=None):
    """float64 W[users] . URM, dense [len(users), items]"""
    W = sps.csr_matrix(W, dtype=np.float64)
    if users is not None:
        W = W[np.asarray(users)]
    return np.asarray(W.dot(sps.csr_matrix(urm, dtype=np.float64)).todense())


def terms(urm, W, users=None):
    """the number of stored products behind every score: pattern(W[users]) . pattern(URM)"""
    Wp, Xp = sps.csr_matrix(W, dtype=np.float64, copy=True), sps.csr_matrix(urm, dtype=np.float64, copy=True)
    Wp.data[:] = 1.0
    Xp.data[:] = 1.0
    return scores(Xp, Wp, users)


def ranked_lists(s, cutoff):
    """the project's ranking of dense scores: descending, ties to the smaller item id; -inf never listed"""
    order = np.argsort(-s, axis=1, kind="stable")
    ranked = np.take_along_axis(s, order, axis=1)
    return [order[r, :cutoff][np.isfinite(ranked[r, :cutoff])].tolist() for r in range(s.shape[0])]


class HelperEngine(H.HelperEngine):
    """Stands where ganmf_amd.engine.Engine does in UserKNNCFRecommender: the float64 fit on what side 0 holds at that moment, the
    scores from W and what side 0 holds when they are asked for"""

    def userknn_fit(self, kind, topk, shrink=0.0, p0=1.0, p1=1.0, den_a=None, den_b=None):
        self.fit_args = dict(kind=kind, topk=topk, shrink=shrink, p0=p0, p1=p1, den_a=den_a, den_b=den_b)
        self.conf_at_fit = dict(self.conf)
        X = H.dense64(self.conf[0]).T      # side 0 is users x items: the targets are its rows
        self.W = H.w_sparse(H.similarity_dense(X, kind, shrink, p0, p1, den_a, den_b), topk)
        self.user_matrix = True
        return self.W.nnz

    def itemknn_fit(self, *args, **kw):
        raise AssertionError("a user-based model fits through userknn_fit")

    def item_similarity(self):
        raise AssertionError("a user-based model reads user_similarity")

    def set_item_similarity(self, W):
        raise AssertionError("a user-based model uploads through set_user_similarity")

    def user_similarity(self):
        return sps.csr_matrix(self.W, dtype=np.float32)

    def set_user_similarity(self, W):
        assert W.shape == (self.num_users, self.num_users)
        self.W = sps.csr_matrix(W, dtype=np.float64)

    def scores(self, ids, transposed=False):
        assert not transposed
        s = scores(self.conf[0], self.W, ids).astype(np.float32)
        if self.filter is not None:
            keep = np.zeros(self.num_items, dtype=bool)
            keep[np.asarray(self.filter)] = True
            s[:, ~keep] = -np.inf
        return s
