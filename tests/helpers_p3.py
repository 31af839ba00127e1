"""P3alpha / RP3beta in numpy float64, restated from the reference's GraphBased/P3alphaRecommender.py:52-141 and
RP3betaRecommender.py:49-151 (steps: transition weights, the walk's rows, top-K per row, row normalisation, top-K per column) under
this project's tie rule (among equal values the smaller item id is selected; `larger_id=True` gives the opposite rule, which the
fixture tool uses to prove a case tie-free), plus a HelperEngine: what the device kernels and the host classes are checked against.
Nothing here imports the reference.  Every matrix is scipy CSR with W[i, j]: row = source item i, column = target item j, the
reference's W_sparse layout; the functions keep the dtype they are given, so the selections can be applied to float32 bytes."""
import numpy as np
import scipy.sparse as sps

from tests import helpers_itemknn as HK

EPS32 = HK.EPS32
scores = HK.scores


def canonical(urm):
    """CSR copy with sorted indices and summed duplicates; STORED zeros are kept (they count in an item's degree)"""
    m = sps.csr_matrix(urm, copy=True)
    m.sum_duplicates()
    m.sort_indices()
    return m


def transition_terms(urm, alpha, beta=None):
    """(row_scale, pui_by_item, col_scale) in float64: row_scale[i] = (1 / deg_i)^alpha (0 where deg_i = 0), pui_by_item the
    items x users CSR with (x_ui / sum_j |x_uj|)^alpha at the stored entries of urm^T, col_scale[j] = deg_j^-beta (0 where
    deg_j = 0; None without beta).  deg counts stored entries."""
    m = canonical(urm)
    m = sps.csr_matrix((m.data.astype(np.float64), m.indices, m.indptr), shape=m.shape)
    n_users, n_items = m.shape
    data = np.zeros_like(m.data)
    for u in range(n_users):
        a, b = m.indptr[u], m.indptr[u + 1]
        norm = np.abs(m.data[a:b]).sum()
        data[a:b] = m.data[a:b] / (norm if norm != 0 else 1.0)
    deg = np.bincount(m.indices, minlength=n_items).astype(np.float64)
    row_scale = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)
    if alpha != 1.0:
        data = data ** float(alpha)
        row_scale = np.where(deg > 0, row_scale ** float(alpha), 0.0)
    col_scale = None if beta is None else np.where(deg > 0, np.maximum(deg, 1.0) ** (-float(beta)), 0.0)
    by_item = sps.csr_matrix((data, m.indices, m.indptr), shape=m.shape).tocsc()
    by_item.sort_indices()
    return row_scale, sps.csr_matrix((by_item.data, by_item.indices, by_item.indptr), shape=(n_items, n_users)), col_scale


def rows_sparse(row_scale, pui_by_item, col_scale=None, dtype=np.float64):
    """the walk before any selection, CSR [n, n] of `dtype`: w[i, j] = sum over the users u STORED in row i of pui_by_item of
    row_scale[i] * pui[u, j], times col_scale[j], the diagonal 0.  dtype=np.float32 takes the product in float32."""
    P = sps.csr_matrix(pui_by_item, dtype=dtype)
    n = P.shape[0]
    piu = sps.csr_matrix((np.repeat(np.asarray(row_scale, dtype=dtype), np.diff(P.indptr)), P.indices, P.indptr), shape=P.shape)
    w = sps.csr_matrix(piu.dot(sps.csr_matrix(P.T)))
    if col_scale is not None:
        w = sps.csr_matrix(w.dot(sps.diags(np.asarray(col_scale, dtype=dtype))))
    c = w.tocoo()
    keep = (c.row != c.col) & (c.data != 0)
    w = sps.csr_matrix((c.data[keep], (c.row[keep], c.col[keep])), shape=(n, n), dtype=dtype)
    w.sort_indices()
    assert w.dtype == dtype and w.shape == (n, n)
    return w


def rows_dense(row_scale, pui_by_item, col_scale=None, dtype=np.float64):
    """rows_sparse as a dense array: the w values before the selection"""
    return rows_sparse(row_scale, pui_by_item, col_scale, dtype).toarray()


def _order(values, ids, larger_id):
    """positions by descending value, ties by ascending (or descending) id"""
    return np.lexsort((-ids if larger_id else ids, -values))


def select_rows(w, topk, larger_id=False):
    """Per row i: of the min(topk, n) largest of ALL n values (the zeros that are not stored included), those that are not zero.
    CSR of w's dtype, columns ascending."""
    w = sps.csr_matrix(w)
    n = w.shape[1]
    k = min(int(topk), n)
    indptr, indices, data = [0], [], []
    for i in range(w.shape[0]):
        a, b = w.indptr[i], w.indptr[i + 1]
        ids, vals = w.indices[a:b], w.data[a:b]
        keep = vals != 0
        ids, vals = ids[keep], vals[keep]
        order = _order(vals, ids, larger_id)
        ids, vals = ids[order], vals[order]
        n_pos = int((vals > 0).sum())
        n_zero = n - len(vals)
        take = np.arange(min(n_pos, k))      # the positive values, then the zeros (dropped), then the negative values
        if k > n_pos + n_zero:
            take = np.concatenate([take, np.arange(n_pos, n_pos + (k - n_pos - n_zero))])
        ids, vals = ids[take], vals[take]
        asc = np.argsort(ids)
        indices.append(ids[asc])
        data.append(vals[asc])
        indptr.append(indptr[-1] + len(take))
    return sps.csr_matrix((np.concatenate(data) if data else np.zeros(0, w.dtype), np.concatenate(indices) if indices else
                           np.zeros(0, np.int32), np.array(indptr)), shape=w.shape)


def normalize_rows(R):
    """every row divided by the sum of the absolute values of its entries (float64 sums); empty rows stay empty"""
    R = sps.csr_matrix(R, dtype=np.float64, copy=True)
    for i in range(R.shape[0]):
        a, b = R.indptr[i], R.indptr[i + 1]
        s = np.abs(R.data[a:b]).sum()
        if s > 0:
            R.data[a:b] /= s
    return R


def select_columns(R, topk, larger_id=False):
    """Per column j: the min(topk, n) largest of its NON-ZERO entries (Base/Recommender_utils.py:48-115).  Moves values only:
    CSR of R's dtype, the same bytes."""
    C = sps.csc_matrix(R)
    C.sort_indices()
    k = min(int(topk), C.shape[0])
    rows, cols, vals = [], [], []
    for j in range(C.shape[1]):
        a, b = C.indptr[j], C.indptr[j + 1]
        ids, v = C.indices[a:b], C.data[a:b]
        keep = v != 0
        ids, v = ids[keep], v[keep]
        order = _order(v, ids, larger_id)[:k]
        rows.append(ids[order])
        cols.append(np.full(len(order), j, dtype=np.int64))
        vals.append(v[order])
    out = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=C.shape, dtype=C.dtype)
    out.sort_indices()
    return out


def walk(row_scale, pui_by_item, col_scale, topk, normalize, col_topk, dtype=np.float64, larger_id=False):
    """steps 3 to 5 from given transition terms; col_topk = 0: no column selection"""
    R = select_rows(rows_sparse(row_scale, pui_by_item, col_scale, dtype), topk, larger_id)
    if normalize:
        R = normalize_rows(R).astype(dtype)
    return select_columns(R, col_topk, larger_id) if col_topk else R


def fit(urm, topK=100, alpha=1.0, beta=None, normalize_similarity=False, dtype=np.float64, larger_id=False):
    """W_sparse (CSR) of the reference's fit() after its min_rating / implicit step, under the project's tie rule.  dtype=np.float32:
    the transition terms rounded to float32 and the product taken in float32."""
    row_scale, pui, col_scale = transition_terms(urm, alpha, beta)
    if dtype != np.float64:
        row_scale, pui = row_scale.astype(dtype), pui.astype(dtype)
        col_scale = None if col_scale is None else col_scale.astype(dtype)
    k = min(int(topK), sps.csr_matrix(urm).shape[1])
    return walk(row_scale, pui, col_scale, k, normalize_similarity, k, dtype, larger_id)


def apply_min_rating(urm, min_rating, implicit):
    """step 1 on a copy: entries below min_rating removed when min_rating > 0, and only then `implicit` sets ones"""
    m = sps.csr_matrix(urm, dtype=np.float32, copy=True)
    if min_rating > 0:
        m.data[m.data < min_rating] = 0
        m.eliminate_zeros()
        if implicit:
            m.data[:] = 1.0
    return m


class HelperEngine(HK.HelperEngine):
    """Stands where ganmf_amd.engine.Engine does in the P3 classes, computing with this module in float64 from what the class
    uploaded and recording it"""

    def p3_fit(self, topk, row_scale, col_scale=None, normalize=False, col_topk=None):
        self.fit_args = dict(topk=topk, row_scale=row_scale, col_scale=col_scale, normalize=normalize, col_topk=col_topk)
        self.conf_at_fit = dict(self.conf)
        ck = topk if col_topk is None else col_topk
        self.W = walk(np.asarray(row_scale, dtype=np.float64), sps.csr_matrix(self.conf[1], dtype=np.float64),
                      None if col_scale is None else np.asarray(col_scale, dtype=np.float64), topk, normalize, ck)
        return self.W.nnz
