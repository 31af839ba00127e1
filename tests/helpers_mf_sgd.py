"""MF-BPR and FunkSVD restated on the host in float64, for the tests of ganmf_mf_sgd_* and of the MatrixFactorization_*_Cython
classes: the reference's two epochs (MatrixFactorization/Cython/MatrixFactorization_Cython_Epoch.pyx:287-389, :614-696) with its
adaptive_gradient (:760-798), in two summation orders; the device's counter-based sampler (csrc/counter_draw.hpp); glibc's rand() with
the reference's own two samplers on top of it (:803-910), which is how tools/make_mf_sgd_fixture.py predicts the sample list of a
seeded reference run; and a stand-in for the engine.
Plain Python floats: every product and sum rounds once."""
import math

import numpy as np
import scipy.sparse as sps

from tests import helpers_ials as HI
from tests import helpers_slim_bpr as HS

WAVE = 64          # csrc/mf_sgd.hpp MF_SGD_WAVE
GAMMA, BETA_1, BETA_2 = 0.995, 0.9, 0.999
MODES = ["sgd", "adagrad", "rmsprop", "adam"]


def f32(x):
    """x as a C float member holds it, widened back to a double"""
    return float(np.float32(x))


# ---- the two summation orders -----------------------------------------------------------------------------------------------------------
def wave_sum(part):
    """the xor butterfly of mf_wave_sum over 64 values, offsets 32, 16, ..., 1; lane 0's result (every lane holds the same one)"""
    part = list(part)
    o = WAVE // 2
    while o > 0:
        part = [part[l] + part[l ^ o] for l in range(WAVE)]
        o //= 2
    return part[0]


def strided_sum(terms):
    """lane l adds the terms l, l + 64, ... in ascending order from 0.0, then the butterfly"""
    part = [0.0] * WAVE
    for q, t in enumerate(terms):
        part[q % WAVE] += t
    return wave_sum(part)


def running_sum(terms, start=0.0):
    x = start
    for t in terms:
        x += t
    return x


# ---- the update -------------------------------------------------------------------------------------------------------------------------
class Trainer(object):
    """The reference's epoch object restated.  apply(users, items, third, batch_size) runs the list in mini-batches (the last one may
    be shorter; the batch scalar is the mean over the samples the batch has).  third: the negative items (MF_BPR) or the ratings
    (FUNK_SVD).  tree = False is R_seq: the prediction and the batch scalar as running sums in the reference's order (the FunkSVD
    prediction starts from the bias sum).  tree = True is R_tree: both in the device's order (strided_sum; the FunkSVD prediction is
    the bias sum plus the finished dot product).  The rates are used as given: round them with f32 first."""

    def __init__(self, algorithm, user_factors, item_factors, use_bias=False, sgd_mode="sgd", learning_rate=1e-3, user_reg=0.0,
                 positive_reg=0.0, negative_reg=0.0, bias_reg=0.0, tree=False):
        assert algorithm in ("MF_BPR", "FUNK_SVD") and sgd_mode in MODES
        self.bpr, self.use_bias, self.mode, self.tree = algorithm == "MF_BPR", bool(use_bias), sgd_mode, tree
        self.lr, self.user_reg, self.pos_reg, self.neg_reg, self.bias_reg = (float(v) for v in (
            learning_rate, user_reg, positive_reg, negative_reg, bias_reg))
        self.W = [[float(v) for v in row] for row in np.asarray(user_factors, dtype=np.float64)]
        self.H = [[float(v) for v in row] for row in np.asarray(item_factors, dtype=np.float64)]
        self.k = len(self.W[0])
        nu, ni = len(self.W), len(self.H)
        self.ub, self.ib, self.gb = [0.0] * nu, [0.0] * ni, [0.0]
        # st0 / st1 of every parameter: [cache or first moment, second moment] per element
        self.sW = [[[0.0, 0.0] for _ in range(self.k)] for _ in range(nu)]
        self.sH = [[[0.0, 0.0] for _ in range(self.k)] for _ in range(ni)]
        self.sub, self.sib, self.sgb = [[0.0, 0.0] for _ in range(nu)], [[0.0, 0.0] for _ in range(ni)], [[0.0, 0.0]]
        self.b1p, self.b2p = BETA_1, BETA_2
        self.scalars = []

    def adapt(self, g, st):
        if self.mode == "adagrad":
            st[0] += g * g
            return g / (math.sqrt(st[0]) + 1e-8)
        if self.mode == "rmsprop":
            st[0] = st[0] * GAMMA + (1.0 - GAMMA) * (g * g)
            return g / (math.sqrt(st[0]) + 1e-8)
        if self.mode == "adam":
            st[0] = st[0] * BETA_1 + (1.0 - BETA_1) * g
            st[1] = st[1] * BETA_2 + (1.0 - BETA_2) * (g * g)
            m1 = st[0] / (1.0 - self.b1p)
            m2 = st[1] / (1.0 - self.b2p)
            return m1 / (math.sqrt(m2) + 1e-8)
        return g

    def term(self, u, i, third):
        Wu, Hi = self.W[u], self.H[i]
        if self.bpr:
            Hj = self.H[third]
            prods = [Wu[f] * (Hi[f] - Hj[f]) for f in range(self.k)]
            x = strided_sum(prods) if self.tree else running_sum(prods)
            return 1.0 / (1.0 + math.exp(x))
        prods = [Wu[f] * Hi[f] for f in range(self.k)]
        bias = (self.gb[0] + self.ub[u]) + self.ib[i] if self.use_bias else 0.0
        if self.tree:
            x = strided_sum(prods)
            prediction = bias + x if self.use_bias else x
        else:
            prediction = running_sum(prods, bias)
        return third - prediction

    def batch(self, users, items, third):
        n = len(users)
        terms = [self.term(users[t], items[t], third[t]) for t in range(n)]
        s = (strided_sum(terms) if self.tree else running_sum(terms)) / float(n)
        self.scalars.append(s)
        lr = self.lr
        if not self.bpr and self.use_bias:
            g = s - self.bias_reg * self.gb[0]
            g = self.adapt(g, self.sgb[0])
            self.gb[0] += lr * g
        for t in range(n):
            u, i = users[t], items[t]
            Wu, Hi = self.W[u], self.H[i]
            if self.bpr:
                j = third[t]
                Hj = self.H[j]
                for f in range(self.k):
                    h_i, h_j, w_u = Hi[f], Hj[f], Wu[f]
                    gi = s * w_u - self.pos_reg * h_i
                    gj = s * (-w_u) - self.neg_reg * h_j
                    gu = s * (h_i - h_j) - self.user_reg * w_u
                    gi = self.adapt(gi, self.sH[i][f])
                    gj = self.adapt(gj, self.sH[j][f])
                    gu = self.adapt(gu, self.sW[u][f])
                    Wu[f] += lr * gu
                    Hi[f] += lr * gi
                    Hj[f] += lr * gj
                continue
            if self.use_bias:
                gbi = s - self.bias_reg * self.ib[i]
                gbu = s - self.bias_reg * self.ub[u]
                gbi = self.adapt(gbi, self.sib[i])
                gbu = self.adapt(gbu, self.sub[u])
                self.ib[i] += lr * gbi
                self.ub[u] += lr * gbu
            for f in range(self.k):
                h_i, w_u = Hi[f], Wu[f]
                gi = s * w_u - self.pos_reg * h_i
                gu = s * h_i - self.user_reg * w_u
                gi = self.adapt(gi, self.sH[i][f])
                gu = self.adapt(gu, self.sW[u][f])
                Hi[f] += lr * gi
                Wu[f] += lr * gu
        if self.mode == "adam":
            self.b1p *= BETA_1
            self.b2p *= BETA_2

    def apply(self, users, items, third, batch_size):
        users, items = [int(v) for v in users], [int(v) for v in items]
        third = [int(v) for v in third] if self.bpr else [float(v) for v in third]
        for first in range(0, len(users), int(batch_size)):
            last = min(first + int(batch_size), len(users))
            self.batch(users[first:last], items[first:last], third[first:last])
        return self

    def params(self):
        return {"USER_factors": np.array(self.W), "ITEM_factors": np.array(self.H), "USER_bias": np.array(self.ub),
                "ITEM_bias": np.array(self.ib), "GLOBAL_bias": np.array(self.gb)}

    def state(self, which):
        pick = lambda rows: np.array([[e[which] for e in row] for row in rows])
        flat = lambda rows: np.array([e[which] for e in rows])
        return {"USER_factors": pick(self.sW), "ITEM_factors": pick(self.sH), "USER_bias": flat(self.sub), "ITEM_bias": flat(self.sib),
                "GLOBAL_bias": flat(self.sgb)}


MEMBERS = ("USER_factors", "ITEM_factors", "USER_bias", "ITEM_bias", "GLOBAL_bias")


def blocks(trainer):
    """every float64 value of the state as (name, array): the parameters and both optimiser arrays"""
    out = []
    for label, d in (("params", trainer.params()), ("state0", trainer.state(0)), ("state1", trainer.state(1))):
        out.extend((label + "." + n, d[n]) for n in MEMBERS)
    return out


# ---- the device's sampler ---------------------------------------------------------------------------------------------------------------
def per_epoch(algorithm, profiles, batch_size):
    base = profiles.shape[0] if algorithm == "MF_BPR" else profiles.nnz
    return (base // int(batch_size) + 1) * int(batch_size)


def draw(algorithm, seed, epoch, n_epochs, profiles, batch_size, quota=0.0):
    """the samples of the epochs [epoch, epoch + n_epochs) as draw_kernel (csrc/counter_draw.hpp) draws them: (users, items, neg_items) int32 for MF_BPR,
    (users, items, ratings float64) for FUNK_SVD"""
    m = sps.csr_matrix(profiles)
    m.sort_indices()
    n_users, n_items = m.shape
    lengths = np.diff(m.indptr)
    eligible = np.flatnonzero((lengths > 0) & (lengths < n_items))
    per = per_epoch(algorithm, m, batch_size)
    users, items, third = [], [], []
    for e in range(epoch, epoch + n_epochs):
        for index in range(per):
            u, i, j = HS.draw_one(seed, e, index, m.indptr, m.indices, n_users, n_items, eligible)
            users.append(u)
            if algorithm == "MF_BPR":
                items.append(i)
                third.append(j)
                continue
            key = HS.mix(HS.mix(HS.mix(seed & HS.M64) ^ e) ^ index)
            positive = quota == 0.0 or float(HS.below(HS.word(key, 3, 0), 1 << 31)) <= quota * 2147483647.0
            if positive:
                lo = m.indptr[u]
                q = lo + HS.below(HS.word(key, 1, 0), int(m.indptr[u + 1] - lo))
                assert m.indices[q] == i
                items.append(i)
                third.append(float(m.data[q]))
            else:
                items.append(j)
                third.append(0.0)
    return (np.array(users, dtype=np.int32), np.array(items, dtype=np.int32),
            np.array(third, dtype=np.int32 if algorithm == "MF_BPR" else np.float64))


# ---- glibc's rand() and the reference's samplers on it ------------------------------------------------------------------------------------
RAND_MAX = 2147483647


class GlibcRand(object):
    """rand() / srand() of glibc (random_r.c, TYPE_3): r[i] = r[i - 31] + r[i - 3] over 32-bit words, seeded by the Lehmer generator
    16807 x mod (2^31 - 1), the first 310 outputs discarded; rand() is the word shifted right by one"""

    def __init__(self, seed):
        seed = int(seed) & 0xFFFFFFFF
        r = [seed if seed != 0 else 1]
        for _ in range(30):
            r.append((16807 * r[-1]) % 2147483647)
        r.extend(r[0:3])
        for i in range(34, 344):
            r.append((r[i - 31] + r[i - 3]) & 0xFFFFFFFF)
        self.r = r[-31:]

    def rand(self):
        v = (self.r[-31] + self.r[-3]) & 0xFFFFFFFF
        self.r.append(v)
        del self.r[0]
        return v >> 1


def reference_samples(algorithm, rng, n, profiles, quota=0.0):
    """n samples as sampleBPR_Cython / sampleMSE_Cython draw them from `rng`, in order"""
    m = sps.csr_matrix(profiles)
    m.sort_indices()
    n_users, n_items = m.shape
    users, items, third = [], [], []
    for _ in range(n):
        seen = 0
        while seen == 0 or seen == n_items:
            u = rng.rand() % n_users
            lo, hi = m.indptr[u], m.indptr[u + 1]
            seen = hi - lo
        profile = m.indices[lo:hi]
        positive = True
        if algorithm == "FUNK_SVD" and quota != 0.0:
            positive = float(rng.rand()) <= quota * RAND_MAX
        if algorithm == "MF_BPR" or positive:
            q = rng.rand() % seen
            i, r = int(profile[q]), float(m.data[lo + q])
        if algorithm == "MF_BPR" or not positive:
            while True:
                j = rng.rand() % n_items
                if j not in profile:
                    break
        users.append(u)
        if algorithm == "MF_BPR":
            items.append(i)
            third.append(j)
        else:
            items.append(i if positive else j)
            third.append(r if positive else 0.0)
    return (np.array(users, dtype=np.int32), np.array(items, dtype=np.int32),
            np.array(third, dtype=np.int32 if algorithm == "MF_BPR" else np.float64))


# ---- a stand-in for the engine ------------------------------------------------------------------------------------------------------------
class HelperEngine(HI.HelperEngine):
    """Stands where ganmf_amd.engine.Engine does in the MatrixFactorization_*_Cython classes, training with this module (R_seq on the
    device sampler's restated samples) and recording what the class asked for"""

    def mf_sgd_init(self, algorithm, profiles, user_factors, item_factors, use_bias=False, sgd_mode="sgd", learning_rate=1e-3,
                    user_reg=0.0, item_reg=0.0, positive_reg=0.0, negative_reg=0.0, bias_reg=0.0, negative_interactions_quota=0.0, seed=0):
        self.init_args = dict(algorithm=algorithm, use_bias=use_bias, sgd_mode=sgd_mode, learning_rate=learning_rate, user_reg=user_reg,
                              item_reg=item_reg, positive_reg=positive_reg, negative_reg=negative_reg, bias_reg=bias_reg,
                              negative_interactions_quota=negative_interactions_quota, seed=seed)
        self.profiles = sps.csr_matrix(profiles)
        assert self.profiles.has_canonical_format and self.profiles.dtype == np.float64
        self.initial = (np.array(user_factors), np.array(item_factors))
        k = self.t[100].shape[1] - 2 * int(bool(use_bias))
        assert self.initial[0].shape == (self.t[100].shape[0], k) and self.initial[1].shape == (self.t[101].shape[0], k)
        self.trainer = Trainer(algorithm, user_factors, item_factors, use_bias, sgd_mode, learning_rate, user_reg, positive_reg,
                               negative_reg, bias_reg)
        self.algorithm, self.quota, self.seed, self.epoch, self.routes, self.publishes = algorithm, negative_interactions_quota, seed, 0, [], 0

    def mf_sgd_epochs(self, n_epochs=1, batch_size=1000, route=0):
        self.trainer.apply(*draw(self.algorithm, self.seed, self.epoch, n_epochs, self.profiles, batch_size, self.quota), batch_size=batch_size)
        self.epoch += n_epochs
        self.routes.append((batch_size, route))
        return 1

    def mf_sgd_state(self):
        return {"params": self.trainer.params(), "state0": self.trainer.state(0), "state1": self.trainer.state(1),
                "beta_powers": np.array([self.trainer.b1p, self.trainer.b2p]), "epoch": self.epoch}

    def mf_sgd_publish(self):
        p = self.trainer.params()
        U, V = p["USER_factors"], p["ITEM_factors"]
        if self.trainer.use_bias:
            U = np.hstack([U, (p["USER_bias"] + p["GLOBAL_bias"][0])[:, None], np.ones((U.shape[0], 1))])
            V = np.hstack([V, np.ones((V.shape[0], 1)), p["ITEM_bias"][:, None]])
        self.set_tensor(100, U)
        self.set_tensor(101, V)
        self.publishes += 1

    def scores(self, ids, transposed=False):
        return self.t[100][np.asarray(ids)].dot(self.t[101].T)
