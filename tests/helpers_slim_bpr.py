"""SLIM-BPR restated on the host in float64, for the tests of ganmf_slim_bpr_* and of the SLIM_BPR_Cython class: the reference's epoch
(SLIM_BPR/Cython/SLIM_BPR_Cython_Epoch.pyx:198-347: four optimisers x dense / symmetric storage), get_S with the class's column top-K
(:373-421, SLIM_BPR_Cython.py:188-197) under the device's tie rule, and the device's counter-based sampler (csrc/counter_draw.hpp).
Plain Python floats: every product and sum rounds once, in the reference's order."""
import math

import numpy as np
import scipy.sparse as sps

from tests import helpers_itemknn as HK

M64 = (1 << 64) - 1
ATTEMPTS = 64      # csrc/counter_draw.hpp DRAW_ATTEMPTS
THREADS = 256      # csrc/slim_bpr.hpp SLIM_THREADS


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def mix(z):
    """the output function of splitmix64"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word(key, stream, attempt):
    return mix(key ^ ((stream << 32) | attempt))


def below(w, m):
    return ((w >> 32) * m) >> 32


def draw_one(seed, epoch, index, indptr, indices, n_users, n_items, eligible):
    key = mix(mix(mix(seed & M64) ^ epoch) ^ index)
    u = -1
    for a in range(ATTEMPTS):
        c = below(word(key, 0, a), n_users)
        if 0 < indptr[c + 1] - indptr[c] < n_items:
            u = c
            break
    if u < 0:
        u = int(eligible[below(word(key, 0, ATTEMPTS), len(eligible))])
    profile = indices[indptr[u]:indptr[u + 1]]
    i = int(profile[below(word(key, 1, 0), len(profile))])
    seen = set(int(s) for s in profile)
    j = -1
    for a in range(ATTEMPTS):
        c = below(word(key, 2, a), n_items)
        if c not in seen:
            j = c
            break
    if j < 0:      # the k-th item outside the ascending profile
        j = below(word(key, 2, ATTEMPTS), n_items - len(profile))
        for s in profile:
            if s <= j:
                j += 1
            else:
                break
    return u, i, j


def draw(seed, epoch, n_epochs, profiles):
    """(users, pos, neg) of the epochs [epoch, epoch + n_epochs): n_users + 1 samples each"""
    m = sps.csr_matrix(profiles)
    m.sort_indices()
    n_users, n_items = m.shape
    lengths = np.diff(m.indptr)
    eligible = np.flatnonzero((lengths > 0) & (lengths < n_items))
    out = [draw_one(seed, e, k, m.indptr, m.indices, n_users, n_items, eligible)
           for e in range(epoch, epoch + n_epochs) for k in range(n_users + 1)]
    return tuple(np.array(v, dtype=np.int32) for v in zip(*out)) if out else tuple(np.zeros(0, dtype=np.int32) for _ in range(3))


# ---- the update -----------------------------------------------------------------------------------------------------------------------
class Trainer(object):
    """The reference's epoch object restated: apply(users, pos, neg) runs the samples one after another.
    tree_sum = False: the profile sum in the reference's order (ascending s, one running sum); True: in the device's (thread t of 256
    adds the entries t, t + 256, ...; the 256 partial sums by a binary tree).  Both are float64 sums of the same terms."""

    def __init__(self, profiles, symmetric, sgd_mode, learning_rate, lambda_i, lambda_j, gamma=0.995, beta_1=0.9, beta_2=0.999,
                 tree_sum=False):
        m = sps.csr_matrix(profiles)
        m.sort_indices()
        self.indptr, self.indices = m.indptr, m.indices
        self.n = m.shape[1]
        self.symmetric, self.mode = bool(symmetric), sgd_mode
        self.lr, self.li, self.lj = float(learning_rate), float(lambda_i), float(lambda_j)
        self.gamma, self.b1, self.b2 = float(gamma), float(beta_1), float(beta_2)
        self.b1p, self.b2p = self.b1, self.b2
        self.T = [[0.0] * self.n for _ in range(self.n)]      # symmetric: only T[max][min] is used
        self.c0 = [0.0] * self.n
        self.c1 = [0.0] * self.n
        self.tree_sum = tree_sum
        self.max_upd = 0.0

    def _at(self, a, b):
        return (max(a, b), min(a, b)) if self.symmetric else (a, b)

    def get(self, a, b):
        r, c = self._at(a, b)
        return self.T[r][c]

    def add(self, a, b, v):
        r, c = self._at(a, b)
        self.T[r][c] += v

    def _sum(self, terms):
        if not self.tree_sum:
            x = 0.0
            for t in terms:
                x += t
            return x
        part = [0.0] * THREADS
        for q, t in enumerate(terms):
            part[q % THREADS] += t
        o = THREADS // 2
        while o > 0:
            for t in range(o):
                part[t] += part[t + o]
            o //= 2
        return part[0]

    def sample(self, u, i, j):
        profile = [int(s) for s in self.indices[self.indptr[u]:self.indptr[u + 1]]]
        x = self._sum([self.get(i, s) - self.get(j, s) for s in profile])
        g = 1.0 / (1.0 + math.exp(x))
        if self.mode == "adagrad":
            self.c0[i] += g * g
            self.c0[j] += g * g
            upd = g / (math.sqrt(self.c0[i]) + 1e-8)
        elif self.mode == "rmsprop":
            self.c0[i] = self.c0[i] * self.gamma + (1.0 - self.gamma) * (g * g)
            self.c0[j] = self.c0[j] * self.gamma + (1.0 - self.gamma) * (g * g)
            upd = g / (math.sqrt(self.c0[i]) + 1e-8)
        elif self.mode == "adam":
            self.c0[i] = self.c0[i] * self.b1 + (1.0 - self.b1) * g
            self.c1[i] = self.c1[i] * self.b2 + (1.0 - self.b2) * (g * g)
            h1 = self.c0[i] / (1.0 - self.b1p)
            h2 = self.c1[i] / (1.0 - self.b2p)
            upd = h1 / (math.sqrt(h2) + 1e-8)
            self.c0[j] = self.c0[j] * self.b1 + (1.0 - self.b1) * g
            self.c1[j] = self.c1[j] * self.b2 + (1.0 - self.b2) * (g * g)
        else:
            assert self.mode == "sgd"
            upd = g
        self.max_upd = max(self.max_upd, abs(upd))
        for s in profile:
            if s != i:
                self.add(i, s, self.lr * (upd - self.li * self.get(i, s)))
            if s != j:
                self.add(j, s, -(self.lr * (upd - self.lj * self.get(j, s))))
        if self.mode == "adam":
            self.b1p *= self.b1
            self.b2p *= self.b2
        return x, g, upd

    def apply(self, users, pos, neg):
        for u, i, j in zip(users, pos, neg):
            self.sample(int(u), int(i), int(j))
        return self

    def S(self):
        """dense [n, n] float64, both halves when symmetric"""
        T = np.array(self.T, dtype=np.float64)
        if self.symmetric:
            T = np.tril(T) + np.tril(T, -1).T
        return T

    def state(self):
        return np.array(self.c0), np.array(self.c1)


# ---- get_S and the column top-K ---------------------------------------------------------------------------------------------------------
def topk_lines(M, k):
    """of every ROW of M the k largest (ties to the smaller id), the non-zero ones kept, the rest zero; dense, M's dtype"""
    n = M.shape[1]
    k = min(int(k), n)
    keep = np.argsort(-M, axis=1, kind="stable")[:, :k]
    out = np.zeros_like(M)
    rows = np.repeat(np.arange(M.shape[0]), k)
    out[rows, keep.ravel()] = M[rows, keep.ravel()]
    return out


def get_S(S, topk):
    """the reference's get_S(): the diagonal zeroed, the top-k of every row in float64; then rounded to float32 (dense)"""
    S = np.array(S, dtype=np.float64)
    np.fill_diagonal(S, 0.0)
    return topk_lines(S, topk).astype(np.float32)


def w_sparse(S, topk):
    """W_sparse of the class: similarityMatrixTopK of get_S -- the top-k of every COLUMN, in float32; CSR, the reference's layout"""
    R = get_S(S, topk)
    W = topk_lines(np.ascontiguousarray(R.T), topk).T
    return sps.csr_matrix(W, dtype=np.float32)


# ---- a stand-in for the engine ----------------------------------------------------------------------------------------------------------
class HelperEngine(HK.HelperEngine):
    """Stands where ganmf_amd.engine.Engine does in SLIM_BPR_Cython, training with this module and recording what the class asked for"""

    def slim_bpr_init(self, symmetric=True, sgd_mode="adagrad", learning_rate=1e-4, lambda_i=0.0, lambda_j=0.0, gamma=0.995,
                      beta_1=0.9, beta_2=0.999, seed=0, profiles=None):
        self.init_args = dict(symmetric=symmetric, sgd_mode=sgd_mode, learning_rate=learning_rate, lambda_i=lambda_i, lambda_j=lambda_j,
                              gamma=gamma, beta_1=beta_1, beta_2=beta_2, seed=seed)
        self.profiles = sps.csr_matrix(self.conf[0] if profiles is None else profiles)
        assert self.profiles.has_canonical_format
        self.trainer = Trainer(self.profiles, symmetric, sgd_mode, learning_rate, lambda_i, lambda_j, gamma, beta_1, beta_2)
        self.seed, self.epoch, self.finishes, self.routes = seed, 0, [], []

    def slim_bpr_epochs(self, n_epochs=1, mode=0):
        self.trainer.apply(*draw(self.seed, self.epoch, n_epochs, self.profiles))
        self.epoch += n_epochs
        self.routes.append(mode)
        return 0

    def slim_bpr_finish(self, topk):
        self.finishes.append((self.epoch, topk))
        self.W = sps.csr_matrix(w_sparse(self.trainer.S(), topk), dtype=np.float64)
        return self.W.nnz

    def slim_bpr_state(self):
        c0, c1 = self.trainer.state()
        return {"S": self.trainer.S(), "state0": c0, "state1": c1, "beta_powers": np.array([self.trainer.b1p, self.trainer.b2p]),
                "epoch": self.epoch}
