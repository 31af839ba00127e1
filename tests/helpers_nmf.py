"""numpy restatement of the two solvers of sklearn.decomposition.NMF as the reference's NMFRecommender runs them (alpha_W = alpha_H =
0: no regularisation term), in the float type asked for: what ganmf_nmf_mu / ganmf_nmf_cd / ganmf_nmf_error (ganmf_amd/csrc/nmf_rows.hpp,
lib/abi_nmf.inc) are compared with.  W is [n_users, k], H is [k, n_items].  EPS is float32's, as sklearn's EPSILON, whatever the type
of the arithmetic.  New code; tests/test_nmf_host.py checks it in float64 against sklearn's own float32 results (tests/golden/nmf_tiny.npz)."""
import numpy as np
import scipy.sparse as sps

from tests import helpers_ials as HI

EPS = float(np.finfo(np.float32).eps)
H_FLOOR = float(np.finfo(np.float64).eps)
FROBENIUS, KULLBACK_LEIBLER = 0, 1


def sampled_wh(X, W, H, dtype):
    """(rows, cols, w_i . h_j at every stored entry of the CSR X)"""
    X = sps.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    cols = X.indices
    wh = np.empty(rows.size, dtype=dtype)
    for a in range(0, rows.size, 8192):
        b = min(a + 8192, rows.size)
        wh[a:b] = (W[rows[a:b]] * H[:, cols[a:b]].T).sum(1, dtype=dtype)
    return rows, cols, wh


def divergence(X, W, H, beta, dtype=np.float64):
    """sklearn's _beta_divergence(X, W, H, beta, square_root=True) for a sparse X"""
    X = sps.csr_matrix(X).astype(dtype)
    W, H = np.asarray(W, dtype=dtype), np.asarray(H, dtype=dtype)
    if beta == FROBENIUS:
        norm_x = np.dot(X.data, X.data)
        norm_wh = ((W.T.dot(W)).dot(H) * H).sum(dtype=dtype)
        cross = (np.asarray(X.dot(H.T)) * W).sum(dtype=dtype)
        return float(np.sqrt(max(float(norm_x + norm_wh - 2 * cross), 0.0)))
    _, _, wh = sampled_wh(X, W, H, dtype)
    keep = X.data > EPS
    x, wh = X.data[keep], np.maximum(wh[keep], dtype(EPS))
    r = np.dot(x, np.log(x / wh)) + np.dot(W.sum(0, dtype=dtype), H.sum(1, dtype=dtype)) - x.sum(dtype=dtype)
    return float(np.sqrt(2 * max(float(r), 0.0)))


def _kl_q(X, W, H, dtype):
    rows, cols, wh = sampled_wh(X, W, H, dtype)
    q = (X.data / np.maximum(wh, dtype(EPS))).astype(dtype)
    return sps.csr_matrix((q, X.indices, X.indptr), shape=X.shape)


def mu(X, W, H, beta, n_iter, update_H=True, dtype=np.float64):
    """n_iter iterations of _fit_multiplicative_update (gamma = 1): (W, H) in `dtype`"""
    X = sps.csr_matrix(X).astype(dtype)
    W, H = np.array(W, dtype=dtype), np.array(H, dtype=dtype)
    eps = dtype(EPS)
    XHt = HHt = Hsum = None
    for _ in range(n_iter):
        if beta == FROBENIUS:
            if XHt is None:
                XHt, HHt = np.asarray(X.dot(H.T), dtype=dtype), H.dot(H.T).astype(dtype)
            den = W.dot(HHt).astype(dtype)
            den[den == 0] = eps
            W = (W * (XHt / den)).astype(dtype)
        else:
            if Hsum is None:
                Hsum = H.sum(1, dtype=dtype)
            num = np.asarray(_kl_q(X, W, H, dtype).dot(H.T), dtype=dtype)
            den = Hsum.copy()
            den[den == 0] = eps
            W = (W * (num / den[None, :])).astype(dtype)
        if not update_H:
            continue
        if beta == FROBENIUS:
            num = np.asarray(X.T.dot(W), dtype=dtype).T
            den = (W.T.dot(W)).dot(H).astype(dtype)
            den[den == 0] = eps
        else:
            num = np.asarray(_kl_q(X, W, H, dtype).T.dot(W), dtype=dtype).T
            wsum = W.sum(0, dtype=dtype)
            wsum[wsum == 0] = 1.0
            den = wsum[:, None]
        H = (H * (num / den)).astype(dtype)
        if beta == KULLBACK_LEIBLER:
            H[H < H_FLOOR] = 0.0
        XHt = HHt = Hsum = None
    return W, H


def cd_half(X, W, Ht, perm, dtype):
    """_update_cdnmf_fast on (X, W, H^T) in place, every row at once (the rows are independent): the violation (float64)"""
    G = Ht.T.dot(Ht).astype(dtype)
    B = np.asarray(X.dot(Ht), dtype=dtype)
    violation = 0.0
    for t in perm:
        grad = (W.dot(G[t]) - B[:, t]).astype(dtype)
        pg = np.where(W[:, t] == 0, np.minimum(grad, 0), grad)
        violation += float(np.abs(pg).sum(dtype=np.float64))
        if G[t, t] != 0:
            W[:, t] = np.maximum(W[:, t] - grad / G[t, t], 0).astype(dtype)
    return violation


def cd(X, W, H, perms, update_H=True, dtype=np.float64):
    """one iteration of _fit_coordinate_descent per row of perms [n_iter, 2 if update_H else 1, k]: (W, H, violations [n_iter])"""
    X = sps.csr_matrix(X).astype(dtype)
    Xt = X.T.tocsr()
    W, Ht = np.array(W, dtype=dtype), np.array(np.asarray(H).T, dtype=dtype)
    out = []
    for pm in np.asarray(perms):
        v = cd_half(X, W, Ht, pm[0], dtype)
        if update_H:
            v += cd_half(Xt, Ht, W, pm[1], dtype)
        out.append(v)
    return W, Ht.T.copy(), np.array(out)


def product_error(W, H, W64, H64):
    """largest |W H - W64 H64| relative to the largest |W64 H64|"""
    P = np.asarray(W, np.float64).dot(np.asarray(H, np.float64))
    P64 = np.asarray(W64, np.float64).dot(np.asarray(H64, np.float64))
    return float(np.abs(P - P64).max() / np.abs(P64).max())


def scalar_error(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def case_matrix(n_users, n_items, seed, density=0.15, long_row=40):
    """[n_users, n_items] float32 ratings in {1 .. 5}: row 0 and column 1 without an entry, row 3 with min(long_row, n_items - 1)
    entries (longer than the 16 entries the sparse product's groups take per round), the others at `density`"""
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_users, n_items) < density) * rng.randint(1, 6, (n_users, n_items)).astype(np.float64)
    n_long = min(long_row, n_items - 1)
    m[3] = 0
    m[3, rng.permutation(n_items)[:n_long]] = rng.randint(1, 6, n_long)
    m[0] = 0
    m[:, 1] = 0
    return sps.csr_matrix(m.astype(np.float32))


def start_factors(X, k, seed):
    """a random start as sklearn's init="random" forms it, from a generator of its own: (W [n_users, k], H [k, n_items]) float32"""
    rng = np.random.RandomState(seed)
    avg = np.sqrt(X.mean() / k)
    H = np.abs(avg * rng.standard_normal((k, X.shape[1]))).astype(np.float32)
    W = np.abs(avg * rng.standard_normal((X.shape[0], k))).astype(np.float32)
    return W, H


class NMFHelperEngine(HI.HelperEngine):
    """HelperEngine with the three NMF entries in float64 over the side-0 upload, or -- with `errors` / `violations` -- answering from
    canned sequences without touching the factors: what NMFRecommender's loops are tested against without a device"""

    def __init__(self, n_users, n_items, num_factors, errors=None, violations=None):
        super(NMFHelperEngine, self).__init__(n_users, n_items, num_factors)
        self.k = num_factors
        self.errors = None if errors is None else list(errors)
        self.violations = None if violations is None else list(violations)
        self.calls = []
        self.first_W = self.transform_start = None

    def set_tensor(self, tid, arr):
        super(NMFHelperEngine, self).set_tensor(tid, arr)
        if tid == 100:      # the first upload of W is the fit's start, the last one transform's
            self.first_W = np.array(arr) if self.first_W is None else self.first_W
            self.transform_start = np.array(arr)

    def pure_svd(self, omega, n_iter):
        from tests import helpers_puresvd as HS
        user, item, sigma = HS.pure_svd(self.conf[0], omega, self.k, n_iter, np.float64)
        self.t[100], self.t[101] = user, item
        return sigma.astype(np.float32)

    def _wh(self):
        return self.t[100], self.t[101].T

    def nmf_error(self, beta):
        self.calls.append(("error", beta))
        if self.errors is not None:
            return self.errors.pop(0)
        return divergence(self.conf[0], *self._wh(), beta)

    def nmf_mu(self, beta, n_iter, update_H=True, error=True):
        self.calls.append(("mu", beta, int(n_iter), bool(update_H), bool(error)))
        if self.errors is not None:
            return self.errors.pop(0) if error else None
        W, H = mu(self.conf[0], *self._wh(), beta, n_iter, update_H)
        self.t[100], self.t[101] = W, H.T.copy()
        return divergence(self.conf[0], W, H, beta) if error else None

    def nmf_cd(self, perms, update_H=True):
        pm = np.asarray(perms).reshape(-1, 2 if update_H else 1, self.k)
        self.calls.append(("cd", pm.copy(), bool(update_H)))
        if self.violations is not None:
            return np.array([self.violations.pop(0) for _ in range(pm.shape[0])])
        W, H, v = cd(self.conf[0], *self._wh(), pm, update_H)
        self.t[100], self.t[101] = W, H.T.copy()
        return v
