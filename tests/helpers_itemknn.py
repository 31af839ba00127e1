"""Item-KNN in numpy float64, restated from the reference's Compute_Similarity_Python (Base/Similarity/Compute_Similarity_Python.py:
209-384) under this project's tie rule (among equal values the smaller item id is selected), plus the scores URM . W: what the device
kernels and the host class are checked against.  Nothing here imports the reference."""
import numpy as np
import scipy.sparse as sps

PRODUCT, TANIMOTO, DICE, TVERSKY, SHRINK_ONLY, RAW = range(6)
KIND_NAMES = ["PRODUCT", "TANIMOTO", "DICE", "TVERSKY", "SHRINK_ONLY", "RAW"]
EPS32 = 2.0 ** -24      # half an ulp of float32, relative


def dense64(urm):
    return np.asarray(sps.csr_matrix(urm).todense(), dtype=np.float64)


def similarity_dense(X, kind, shrink=0.0, p0=1.0, p1=1.0, den_a=None, den_b=None):
    """sim64[j, i]: the value of neighbour j for item i before the selection (column i = item i, the reference's layout), float64.
    X: dense [users, items]; den_a / den_b: the per-item terms, as the device receives them."""
    X = np.asarray(X, dtype=np.float64)
    w = X.T.dot(X)      # w[j, i]
    np.fill_diagonal(w, 0.0)
    s = float(shrink) + 1e-6
    a = None if den_a is None else np.asarray(den_a, dtype=np.float64)
    b = None if den_b is None else np.asarray(den_b, dtype=np.float64)
    if kind == PRODUCT:
        return w / (b[:, None] * a[None, :] + s)
    if kind == TANIMOTO:
        return w / (a[None, :] + a[:, None] - w + s)
    if kind == DICE:
        return w / (a[None, :] + a[:, None] + s)
    if kind == TVERSKY:
        return w / (w + (a[None, :] - w) * p0 + (a[:, None] - w) * p1 + s)
    if kind == SHRINK_ONLY:
        return w / float(shrink)
    return w


def select_topk(sim, topk):
    """Per column i: the min(topk, n) largest values, ties to the smaller row id, the zeros among them dropped.  Returns the list of
    (neighbour ids, values) per column, in descending order of value."""
    n = sim.shape[0]
    k = min(int(topk), n)
    out = []
    for i in range(n):
        col = sim[:, i]
        order = np.lexsort((np.arange(n), -col))[:k]      # value descending, then id ascending
        order = order[col[order] != 0.0]
        out.append((order, col[order]))
    return out


def w_sparse(sim, topk):
    """the selected similarities as the reference lays W_sparse out: CSR float64 [n, n], rows = neighbour, columns = item"""
    n = sim.shape[0]
    rows, cols, vals = [], [], []
    for i, (idx, v) in enumerate(select_topk(sim, topk)):
        rows.extend(idx.tolist())
        cols.extend([i] * len(idx))
        vals.extend(v.tolist())
    return sps.csr_matrix((np.array(vals, dtype=np.float64), (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64))),
                          shape=(n, n))


def host_plan(urm, similarity, normalize, shrink, asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0):
    """What the reference decides on the host for one fit: (kind, the matrix the similarity sees as dense float64, p0, p1, den_a,
    den_b) -- the binarisation, the forced normalize=False and the denominators of Compute_Similarity_Python.py:70-95, 233-250."""
    X = dense64(urm)
    if similarity in ("jaccard", "tanimoto", "dice", "tversky"):
        X = _stored_ones(urm)
        den = (X * X).sum(axis=0)
        kind = {"jaccard": TANIMOTO, "tanimoto": TANIMOTO, "dice": DICE, "tversky": TVERSKY}[similarity]
        return kind, X, float(tversky_alpha), float(tversky_beta), den, None
    if normalize:
        norm = np.sqrt((X * X).sum(axis=0))
        if similarity == "asymmetric":
            return PRODUCT, X, 1.0, 1.0, np.power(norm, 2 * asymmetric_alpha), np.power(norm, 2 * (1 - asymmetric_alpha))
        return PRODUCT, X, 1.0, 1.0, norm, norm
    return (SHRINK_ONLY if shrink != 0 else RAW), X, 1.0, 1.0, None, None


def _stored_ones(urm):
    """ones at the STORED entries (an explicit zero counts, as in the reference's useOnlyBooleanInteractions)"""
    m = sps.csr_matrix(urm, copy=True)
    m.data = np.ones_like(m.data)
    return np.asarray(m.todense(), dtype=np.float64)


def fit(urm, topK=50, shrink=100, similarity="cosine", normalize=True, **kw):
    """W_sparse (CSR float64) of the reference's fit() without feature weighting, under the project's tie rule"""
    kind, X, p0, p1, den_a, den_b = host_plan(urm, similarity, normalize, shrink, **kw)
    return w_sparse(similarity_dense(X, kind, shrink, p0, p1, den_a, den_b), topK)


def scores(urm, W):
    """float64 URM . W, dense [users, items]"""
    return np.asarray(sps.csr_matrix(urm, dtype=np.float64).dot(sps.csr_matrix(W, dtype=np.float64)).todense())


class HelperEngine(object):
    """Stands where ganmf_amd.engine.Engine does in ItemKNNCFRecommender, computing with this module in float64 and recording what
    the host class uploads: its host logic can be tested without a device"""

    def __init__(self, n_users, n_items):
        self.num_users, self.num_items = n_users, n_items
        self.conf = {}
        self.conf_at_fit = {}
        self.fit_args = None
        self.W = None
        self.mask_cold = None
        self.filter = None
        self.closed = False

    def set_seen(self, urm):
        self.seen = sps.csr_matrix(urm)

    def set_score_filter(self, items_to_compute=None, mask_cold=False):
        self.filter, self.mask_cold = items_to_compute, mask_cold

    def set_confidence(self, side, csr):
        m = sps.csr_matrix(csr)
        assert m.has_canonical_format
        self.conf[side] = m

    def itemknn_fit(self, kind, topk, shrink=0.0, p0=1.0, p1=1.0, den_a=None, den_b=None):
        self.fit_args = dict(kind=kind, topk=topk, shrink=shrink, p0=p0, p1=p1, den_a=den_a, den_b=den_b)
        self.conf_at_fit = dict(self.conf)
        X = dense64(self.conf[1]).T      # side 1 is items x users
        self.W = w_sparse(similarity_dense(X, kind, shrink, p0, p1, den_a, den_b), topk)
        return self.W.nnz

    def item_similarity(self):
        return sps.csr_matrix(self.W, dtype=np.float32)

    def set_item_similarity(self, W):
        self.W = sps.csr_matrix(W, dtype=np.float64)

    def scores(self, ids, transposed=False):
        assert not transposed
        s = scores(self.conf[0][np.asarray(ids)], self.W).astype(np.float32)
        if self.filter is not None:
            keep = np.zeros(self.num_items, dtype=bool)
            keep[np.asarray(self.filter)] = True
            s[:, ~keep] = -np.inf
        return s

    def close(self):
        self.closed = True
