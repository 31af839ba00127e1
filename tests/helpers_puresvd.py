"""numpy restatement of ganmf_pure_svd (ganmf_amd/csrc/svd_rows.hpp, lib/abi_svd.inc) in the float type asked for: the randomized
truncated SVD of sklearn.utils.extmath.randomized_svd with the device's choices -- every half step orthonormalised by Cholesky-QR
applied twice (inverse Cholesky factor formed, then multiplied), the eigenpairs of the final Gram matrix by a one-sided Jacobi
iteration in round-robin order with the device's thresholds, W = columns / lambda, sigma = the column norms of Z W,
sklearn's sign rule.  New code; tests/test_puresvd_host.py checks it in float64 against sklearn itself."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

from tests import helpers_ials as HI

EIG_MAX_SWEEPS = 30


class Breakdown(ArithmeticError):
    pass


def plan(n_users, n_items, k):
    """(n_random, n_iter, transposed) by sklearn's defaults"""
    return k + 10, (7 if k < 0.1 * min(n_users, n_items) else 4), n_users < n_items


def cholqr2(Y, dtype, stage=""):
    for p in range(2):
        G = Y.T.dot(Y).astype(dtype)
        try:
            Lc = np.linalg.cholesky(G).astype(dtype)
        except np.linalg.LinAlgError:
            raise Breakdown("Cholesky-QR broke down in %s, pass %d" % (stage, p + 1))
        X = sla.solve_triangular(Lc, np.eye(Lc.shape[0], dtype=dtype), lower=True).astype(dtype)
        Y = Y.dot(X.T).astype(dtype)
    return Y


def round_pairs(n, s):
    """the n / 2 pairs of round s of the round-robin tournament over n (even) players, as svd_jacobi_kernel forms them"""
    j = np.arange(1, n // 2)
    a = np.concatenate([[n - 1], (s + j) % (n - 1)])
    b = np.concatenate([[s], (s - j + n - 1) % (n - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_eig(G, dtype):
    """one-sided Jacobi on the symmetric G: (lam [l], A [l, l] with row j = lam_j w_j, sweeps)"""
    A = np.array(G, dtype=dtype)
    l = A.shape[0]
    eps = dtype(2.0 ** -23) if dtype == np.float32 else dtype(2.0 ** -52)
    tol = dtype(np.sqrt(dtype(l))) * eps
    n = (l + 1) // 2 * 2
    done = l < 2
    sweeps = 0
    while not done and sweeps < EIG_MAX_SWEEPS:
        count = 0
        for s in range(n - 1):
            P, Q = round_pairs(n, s)
            keep = Q < l
            P, Q = P[keep], Q[keep]
            X, Y = A[P], A[Q]
            alpha, beta, gamma = (X * X).sum(1, dtype=dtype), (Y * Y).sum(1, dtype=dtype), (X * Y).sum(1, dtype=dtype)
            lim = np.sqrt(alpha) * np.sqrt(beta)
            rot = np.abs(gamma) > dtype(0.25) * tol * lim
            count += int((np.abs(gamma) > tol * lim).sum())
            if not rot.any():
                continue
            P, Q, X, Y = P[rot], Q[rot], X[rot], Y[rot]
            zeta = ((beta[rot] - alpha[rot]) / (dtype(2) * gamma[rot])).astype(dtype)
            t = (np.copysign(dtype(1), zeta) / (np.abs(zeta) + np.sqrt(dtype(1) + zeta * zeta))).astype(dtype)
            c = (dtype(1) / np.sqrt(dtype(1) + t * t)).astype(dtype)
            sn = (c * t).astype(dtype)
            A[P] = c[:, None] * X - sn[:, None] * Y
            A[Q] = sn[:, None] * X + c[:, None] * Y
        done = count == 0
        sweeps += 1
    if not done:
        raise Breakdown("the Jacobi eigensolver did not converge in %d sweeps" % sweeps)
    lam = np.sqrt((A * A).sum(1, dtype=dtype)).astype(dtype)
    return lam, A, sweeps


def pure_svd(urm, omega, k, n_iter, dtype=np.float64):
    """(USER_factors [n_users, k], ITEM_factors [n_items, k], sigma [k]) in `dtype` from the test matrix omega"""
    urm = sps.csr_matrix(urm).astype(dtype)
    n_users, n_items = urm.shape
    transposed = n_users < n_items
    M = urm.T.tocsr() if transposed else urm
    Mt = M.T.tocsr()
    Q = np.array(omega, dtype=dtype)
    assert Q.shape[0] == M.shape[1] and Q.shape[1] >= k
    for it in range(n_iter):
        Q = cholqr2(np.asarray(M.dot(Q), dtype=dtype), dtype, "half step %d (M Q)" % (2 * it))
        Q = cholqr2(np.asarray(Mt.dot(Q), dtype=dtype), dtype, "half step %d (M^T Q)" % (2 * it + 1))
    Q = cholqr2(np.asarray(M.dot(Q), dtype=dtype), dtype, "half step %d (the final range)" % (2 * n_iter))
    Z = np.asarray(Mt.dot(Q), dtype=dtype)
    lam, A, _ = jacobi_eig(Z.T.dot(Z).astype(dtype), dtype)
    order = np.argsort(-lam, kind="stable")[:k]
    lam_k = lam[order]
    if not (lam_k > 0).all():
        raise Breakdown("a singular value is not positive")
    W = (A[order] / lam_k[:, None]).T.astype(dtype)                # [l, k]
    left, right = Q.dot(W).astype(dtype), Z.dot(W).astype(dtype)
    sigma = np.sqrt((right * right).sum(0, dtype=dtype)).astype(dtype)      # |Z w|: second order in the error of w
    if transposed:
        user, item = (right / sigma).astype(dtype), (left * sigma).astype(dtype)
    else:
        user, item = left, right
    neg = user[np.abs(user).argmax(axis=0), np.arange(k)] < 0
    user[:, neg] *= -1
    item[:, neg] *= -1
    return user, item, sigma


def align_signs(U, ref):
    """U with every column's sign chosen by the sign rule applied to `ref`'s arg-max rows (comparison of factor columns)"""
    rows = np.abs(ref).argmax(axis=0)
    s = np.sign(U[rows, np.arange(U.shape[1])]) * np.sign(ref[rows, np.arange(U.shape[1])])
    s[s == 0] = 1
    return U * s


def errors(user, item, sigma, user64, item64, sigma64, transposed):
    """(e_score, e_sigma from `sigma`, e_sigma from the ITEM column norms, largest |U^T U - I| of the orthonormal factor)"""
    user, item = np.asarray(user, np.float64), np.asarray(item, np.float64)
    S, S64 = user.dot(item.T), np.asarray(user64, np.float64).dot(np.asarray(item64, np.float64).T)
    e_score = np.abs(S - S64).max() / np.abs(S64).max()
    s64 = np.asarray(sigma64, np.float64)
    e_sigma = np.abs(np.asarray(sigma, np.float64) - s64).max() / s64[0]
    norms = np.sqrt((item * item).sum(0))
    e_norm = np.abs(norms - s64).max() / s64[0]
    O = item / norms if transposed else user
    e_orth = np.abs(O.T.dot(O) - np.eye(O.shape[1])).max()
    return float(e_score), float(e_sigma), float(e_norm), float(e_orth)


class SVDHelperEngine(HI.HelperEngine):
    """HelperEngine with pure_svd in float64 over the side-0 upload: what PureSVDRecommender's host logic is tested against"""

    def __init__(self, n_users, n_items, num_factors):
        super(SVDHelperEngine, self).__init__(n_users, n_items, num_factors)
        self.k = num_factors
        self.calls = []

    def pure_svd(self, omega, n_iter):
        assert (self.conf[1] != self.conf[0].T).nnz == 0
        self.calls.append((np.shape(omega), int(n_iter)))
        user, item, sigma = pure_svd(self.conf[0], omega, self.k, n_iter, np.float64)
        self.t[100], self.t[101] = user, item
        return sigma.astype(np.float32)


def case_matrix(n_users, n_items, seed, density=0.15, long_row=0):
    """[n_users, n_items] float32 ratings in {1 .. 5}: row 0 without an entry, column 1 without an entry, row 2 with one entry,
    row 3 with `long_row` entries (when asked for), the others at `density`"""
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_users, n_items) < density) * rng.randint(1, 6, (n_users, n_items)).astype(np.float64)
    m[0] = 0
    m[2] = 0
    m[2, n_items // 2] = 4
    if long_row:
        m[3] = 0
        m[3, rng.permutation(n_items)[:long_row]] = rng.randint(1, 6, long_row)
    m[:, 1] = 0
    return sps.csr_matrix(m.astype(np.float32))


def relative_gap(urm, k):
    """(sigma_k - sigma_{k+1}) / sigma_1 of the dense matrix in float64"""
    s = np.linalg.svd(np.asarray(sps.csr_matrix(urm).todense(), dtype=np.float64), compute_uv=False)
    return float((s[k - 1] - s[k]) / s[0])


def gap_matrix(n_users, n_items, k, seed, density=0.08, long_row=0):
    """case_matrix with k stored entries of 400 down to 200 added on the diagonal from (4, 4): k singular values stand clear of the
    bulk of the random part, so that sigma_k - sigma_{k+1} is a sizeable fraction of sigma_1 at any k (a random matrix of this size
    has its singular values 1e-4 sigma_1 apart at k = 250)"""
    m = case_matrix(n_users, n_items, seed, density, long_row).tolil()
    d = np.linspace(400.0, 200.0, k)
    for j in range(k):
        m[4 + j, 4 + j] = d[j]
    return sps.csr_matrix(m.tocsr(), dtype=np.float32)
