"""numpy restatement of implicit-feedback ALS (WRMF): one half sweep and a whole fit(), in the float type asked for.

New code, following the update rule of the reference's IALSRecommender (MatrixFactorization/IALSRecommender.py:137-201):
for a row u with stored columns P(u) and confidences c,  B = Y^T Y + Y_P^T diag(c - 1) Y_P + reg I,  b = Y_P^T c,  x = inv(B) b.
tests/test_ials_host.py checks half_sweep against dense_wls_row, which never forms Y^T Y."""
import numpy as np
import scipy.linalg
import scipy.sparse as sps


def confidence(urm, scaling="linear", alpha=1.0, epsilon=1.0):
    """the confidence of every stored entry, in float32 as the host class forms it"""
    C = sps.csr_matrix(urm, dtype=np.float32, copy=True)
    if scaling == "linear":
        C.data = (1.0 + alpha * C.data).astype(np.float32)
    elif scaling == "log":
        C.data = (1.0 + alpha * np.log(1.0 + C.data / epsilon)).astype(np.float32)
    else:
        raise ValueError(scaling)
    return C


def half_sweep(X, Y, C, reg, dtype=np.float64):
    """X with every row that has a stored entry in the CSR confidence matrix C replaced by its least-squares solution against Y;
    all arithmetic in `dtype`, the inverse as the reference takes it"""
    X = np.array(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    C = sps.csr_matrix(C)
    k = Y.shape[1]
    G = Y.T.dot(Y)
    R = (dtype(reg) * np.eye(k)).astype(dtype)
    for u in range(C.shape[0]):
        lo, hi = C.indptr[u], C.indptr[u + 1]
        if hi == lo:
            continue
        Yp = Y[C.indices[lo:hi]]
        c = C.data[lo:hi].astype(dtype)
        B = G + Yp.T.dot((c - dtype(1))[:, None] * Yp) + R
        X[u] = np.linalg.inv(B).dot(Yp.T.dot(c))
    return X


def system_matrix(Y, C, u, reg, dtype=np.float64):
    """(B, b) of row u of the CSR confidence matrix C in `dtype`: what half_sweep and half_sweep_cholesky solve"""
    Y = np.asarray(Y, dtype=dtype)
    lo, hi = C.indptr[u], C.indptr[u + 1]
    Yp = Y[C.indices[lo:hi]]
    c = C.data[lo:hi].astype(dtype)
    B = Y.T.dot(Y) + Yp.T.dot((c - dtype(1))[:, None] * Yp) + (dtype(reg) * np.eye(Y.shape[1])).astype(dtype)
    return B, Yp.T.dot(c)


def half_sweep_cholesky(X, Y, C, reg, dtype=np.float64):
    """half_sweep with another algorithm behind the same B and b: B = L L^T by np.linalg.cholesky, then L z = b and L^T x = z by
    substitution, all in `dtype`.  A B that is not positive definite raises np.linalg.LinAlgError"""
    X = np.array(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    C = sps.csr_matrix(C)
    k = Y.shape[1]
    G = Y.T.dot(Y)
    R = (dtype(reg) * np.eye(k)).astype(dtype)
    for u in range(C.shape[0]):
        lo, hi = C.indptr[u], C.indptr[u + 1]
        if hi == lo:
            continue
        Yp = Y[C.indices[lo:hi]]
        c = C.data[lo:hi].astype(dtype)
        B = G + Yp.T.dot((c - dtype(1))[:, None] * Yp) + R
        Lc = np.linalg.cholesky(B)
        assert Lc.dtype == dtype
        z = scipy.linalg.solve_triangular(Lc, Yp.T.dot(c), lower=True, check_finite=False)
        x = scipy.linalg.solve_triangular(Lc.T, z, lower=False, check_finite=False)
        assert x.dtype == dtype
        X[u] = x
    return X


# row lengths of edge_matrix: every length around the gather tile of 32 entries (31 .. 33, 63 .. 65, 96, 97), 200, and the mixes of
# empty, short and long rows inside a group of four (the small kernel's workgroup); -1 stands for a twin row
EDGE_TWIN = -1
EDGE_LENGTHS = (0, 1, 2, 31,  32, 33, 63, 64,  65, 96, 97, 0,  0, 0, 0, 0,  200, 0, 0, 1,  1, 0, 0, 200,
                EDGE_TWIN, EDGE_TWIN, EDGE_TWIN, EDGE_TWIN,  EDGE_TWIN, 64, 0, 33,  200, EDGE_TWIN)
EDGE_TWIN_ROWS = tuple(i for i, n in enumerate(EDGE_LENGTHS) if n == EDGE_TWIN)
EDGE_TWIN_LENGTH = 5
EDGE_TAIL_LENGTH = 7


def edge_lengths(n_rows):
    """the row lengths of edge_matrix(n_rows), twin rows with their true length"""
    if n_rows not in (34, 36):
        raise ValueError("edge_matrix has 34 or 36 rows")
    return [EDGE_TWIN_LENGTH if n == EDGE_TWIN else n for n in EDGE_LENGTHS] + [EDGE_TAIL_LENGTH] * (n_rows - 34)


def edge_matrix(n_rows, n_cols=260, seed=0):
    """[n_rows, n_cols] CSR float32 ratings in {1 .. 5} with the row lengths EDGE_LENGTHS (n_rows = 34), or those and two rows of
    length 7 (n_rows = 36).  Each row's columns are a random subset without repeats, in ascending order; the twin rows all hold the
    same five columns with the same five ratings"""
    rng = np.random.RandomState(seed)
    twin_cols = np.sort(rng.permutation(n_cols)[:EDGE_TWIN_LENGTH])
    twin_data = rng.randint(1, 6, EDGE_TWIN_LENGTH)
    indptr, indices, data = [0], [], []
    for u, n in enumerate(edge_lengths(n_rows)):
        if u < 34 and EDGE_LENGTHS[u] == EDGE_TWIN:
            cols, vals = twin_cols, twin_data
        else:
            cols, vals = np.sort(rng.permutation(n_cols)[:n]), rng.randint(1, 6, n)
        indices.extend(cols)
        data.extend(vals)
        indptr.append(len(indices))
    return sps.csr_matrix((np.array(data, dtype=np.float32), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int64)),
                          shape=(n_rows, n_cols))


def dense_wls_row(Y, c_dense, p_dense, reg):
    """argmin_x sum_i c_i (p_i - x . y_i)^2 + reg |x|^2 over ALL items, as one stacked least-squares problem (float64, no normal
    equations and no Y^T Y)"""
    Y = np.asarray(Y, dtype=np.float64)
    k = Y.shape[1]
    w = np.sqrt(np.asarray(c_dense, dtype=np.float64))
    A = np.vstack([w[:, None] * Y, np.sqrt(reg) * np.eye(k)])
    rhs = np.concatenate([w * np.asarray(p_dense, dtype=np.float64), np.zeros(k)])
    return np.linalg.lstsq(A, rhs, rcond=None)[0]


def fit(urm, item_factors, epochs, scaling="linear", alpha=1.0, epsilon=1.0, reg=1e-3, dtype=np.float64):
    """`epochs` epochs from the given ITEM factors and zero USER factors: (USER_factors, ITEM_factors) in `dtype`"""
    C = confidence(urm, scaling, alpha, epsilon)
    Ct = C.T.tocsr()
    V = np.array(item_factors, dtype=dtype)
    U = np.zeros((C.shape[0], V.shape[1]), dtype=dtype)
    for _ in range(epochs):
        U = half_sweep(U, V, C, reg, dtype)
        V = half_sweep(V, U, Ct, reg, dtype)
    return U, V


def row_error(got, ref):
    """largest over the rows of max |got - ref| relative to the row's largest |ref| (rows of zeros: the absolute error)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max(axis=1)
    scale[scale == 0] = 1.0
    return float((np.abs(got - ref).max(axis=1) / scale).max())


def row_errors(got, ref):
    """row_error's figure of every row"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max(axis=1)
    scale[scale == 0] = 1.0
    return np.abs(got - ref).max(axis=1) / scale


class HelperEngine(object):
    """Stands where ganmf_amd.engine.Engine does in IALSRecommender, computing with half_sweep in float64: what the host class's
    loop, snapshots and persistence can be tested against without a device"""

    def __init__(self, n_users, n_items, num_factors):
        self.t = {100: np.zeros((n_users, num_factors)), 101: np.zeros((n_items, num_factors))}
        self.best = {}
        self.conf = {}
        self.sweeps = 0
        self.closed = False

    def set_seen(self, urm):
        pass

    def set_score_filter(self, items_to_compute=None, mask_cold=False):
        self.mask_cold = mask_cold

    def set_tensor(self, tid, arr):
        assert np.shape(arr) == self.t[tid].shape
        self.t[tid] = np.array(arr, dtype=np.float64)

    def get_tensor(self, tid):
        return self.t[tid].astype(np.float32)

    def set_confidence(self, side, csr):
        self.conf[side] = sps.csr_matrix(csr)

    def als_half_sweep(self, side, reg):
        x, y = (100, 101) if side == 0 else (101, 100)
        self.t[x] = half_sweep(self.t[x], self.t[y], self.conf[side], reg)
        self.sweeps += 1

    def snapshot_best(self):
        self.best = {k: v.copy() for k, v in self.t.items()}

    def restore_best(self):
        self.t = {k: v.copy() for k, v in self.best.items()}

    def close(self):
        self.closed = True
