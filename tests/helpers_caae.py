"""Shared pieces of the CAAE tests (not a conftest: imported by the modules that use them).

* CAAERef: a numpy restatement of the model (discriminator, both generators, the three losses, their gradients, plain SGD and an epoch
  driven by GIVEN draws), usable in float64 and float32: every array and scalar is held in `dtype`, so the float32 instance rounds
  where a float32 implementation would.
* abs_d_bounds / abs_g_bounds: per element, the fp64 sum of |terms| behind each gradient -- the same chains with every operand replaced
  by its absolute value, built the way helpers_cfgan.abs_*_bounds are.
* base / u24 / perm_index / perm / users / cdf_draws: a uint64 restatement of the device samplers (a), (b), (c) and (e)."""
import numpy as np

from tests.helpers_cfgan import _M64, mix, mix_np, sigmoid

STREAM_PERM, STREAM_NEG, STREAM_USERS, STREAM_NU, STREAM_ITEMS = 0, 1, 3, 5, 6
FEISTEL_ROUNDS = 6


def log_sigmoid(y):
    return np.minimum(y, y.dtype.type(0)) - np.log1p(np.exp(-np.abs(y)))


class CAAERef(object):
    def __init__(self, weights, lmbda=0.5, beta=1e-4, lr=1e-4, dtype=np.float64):
        """weights: {'D': [P, Q, b], 'G': [W0, b0, ..., Wo, bo], 'G_prime': [...]} (ganmf_amd.CAAE.init_weights' layout)"""
        self.dt = np.dtype(dtype).type
        self.p = {k: [np.array(a, dtype=dtype) for a in v] for k, v in weights.items()}
        self.lmbda, self.beta, self.lr = self.dt(lmbda), self.dt(beta), self.dt(lr)

    # ---- forward ------------------------------------------------------------------------------
    def mlp(self, key, x):
        """[h_0 = x, h_1, ..., r]: every layer's sigmoid output"""
        P = self.p[key]
        h = [np.asarray(x, dtype=self.dt)]
        for l in range(len(P) // 2):
            h.append(sigmoid(h[-1] @ P[2 * l] + P[2 * l + 1]))
        return h

    def scores(self, x):
        return self.mlp("G", x)[-1]

    def cdf(self, key, x):
        """(cdf rows, log sum exp(r)) as CAAE.py:232-235 forms them"""
        e = np.exp(self.mlp(key, x)[-1])
        s = e.sum(axis=1, dtype=self.dt)
        return np.cumsum(e / s[:, None], axis=1, dtype=self.dt), np.log(s)

    # ---- discriminator ----------------------------------------------------------------------------
    def d_grads(self, u, i, j):
        """(loss, [gP, gQ, gb]) of one step on the triples: dense gradients, zero in the rows no triple touches"""
        P, Q, b = self.p["D"]
        u, i, j = (np.asarray(a, dtype=np.int64) for a in (u, i, j))
        B = self.dt(len(u))
        half = self.dt(0.5)
        pu, qi, qj, bi, bj = P[u], Q[i], Q[j], b[i], b[j]
        x = np.sum(pu * (qi - qj), axis=1, dtype=self.dt) + (bi - bj)
        reg = half * (np.sum(pu * pu, dtype=self.dt) + np.sum(qi * qi, dtype=self.dt) + np.sum(qj * qj, dtype=self.dt)
                      + np.sum(bi * bi, dtype=self.dt) + np.sum(bj * bj, dtype=self.dt))
        loss = -np.sum(log_sigmoid(x), dtype=self.dt) / B + self.beta * reg
        c = -np.exp(log_sigmoid(-x)) / B
        gP, gQ, gb = np.zeros_like(P), np.zeros_like(Q), np.zeros_like(b)
        np.add.at(gP, u, c[:, None] * (qi - qj) + self.beta * pu)
        np.add.at(gQ, i, c[:, None] * pu + self.beta * qi)
        np.add.at(gQ, j, -c[:, None] * pu + self.beta * qj)
        np.add.at(gb, i, c + self.beta * bi)
        np.add.at(gb, j, -c + self.beta * bj)
        return loss, [gP, gQ, gb]

    def reward(self, which, users, items):
        P, Q, b = self.p["D"]
        users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
        y = np.einsum("bd,bsd->bs", P[users], Q[items]).astype(self.dt) + b[items]
        one = self.dt(1)
        return log_sigmoid(y - one if which == 0 else one - y)

    # ---- generators -------------------------------------------------------------------------------
    def g_grads(self, which, users, X, nu, items):
        """(loss, grads in tensor order) of one step of G (which = 0: nu = bool [m, I], the subset planes) or G' (which = 1) on the
        users' dense profiles X[users] and the policy items [m, n_s]; gradients include beta * theta"""
        key = "G" if which == 0 else "G_prime"
        P = self.p[key]
        users = np.asarray(users, dtype=np.int64)
        items = np.asarray(items, dtype=np.int64)
        x = np.asarray(X, dtype=self.dt)[users]
        m, n_s = items.shape
        h = self.mlp(key, x)
        r = h[-1]
        lse = np.log(np.sum(np.exp(r), axis=1, dtype=self.dt))
        R = self.reward(which, users, items)
        lsm = np.take_along_axis(r, items, axis=1) - lse[:, None]
        one = self.dt(1)
        pc = (self.lmbda if which == 0 else one) / self.dt(m * n_s)
        ac = one - self.lmbda if which == 0 else self.dt(0)
        loss = -pc * np.sum(lsm * R, dtype=self.dt)
        hit = np.zeros_like(r)
        for s in range(n_s):      # draw order, as the device sums a row's draws
            np.add.at(hit, (np.arange(m), items[:, s]), R[:, s])
        dr = -pc * (hit - R.sum(axis=1, dtype=self.dt)[:, None] * np.exp(r - lse[:, None]))
        if which == 0:
            e = x + (np.asarray(nu, dtype=self.dt) if nu is not None else self.dt(0))
            d = (r - x) * e
            loss = loss + ac * np.sum(d * d, dtype=self.dt)
            dr = dr + self.dt(2) * ac * d * e
        half = self.dt(0.5)
        for a in P:
            loss = loss + self.beta * half * np.sum(a * a, dtype=self.dt)
        grads = [None] * len(P)
        dh = dr
        for l in reversed(range(len(P) // 2)):
            dz = dh * h[l + 1] * (one - h[l + 1])
            grads[2 * l] = h[l].T @ dz + self.beta * P[2 * l]
            grads[2 * l + 1] = dz.sum(axis=0, dtype=self.dt) + self.beta * P[2 * l + 1]
            dh = dz @ P[2 * l].T
        return loss, grads

    # ---- SGD, steps, epoch ---------------------------------------------------------------------------
    def _sgd(self, key, grads):
        self.p[key] = [p - self.lr * g for p, g in zip(self.p[key], grads)]

    def d_step(self, u, i, j):
        loss, grads = self.d_grads(u, i, j)
        self._sgd("D", grads)
        return loss

    def g_step(self, which, users, X, nu, items):
        loss, grads = self.g_grads(which, users, X, nu, items)
        self._sgd("G" if which == 0 else "G_prime", grads)
        return loss

    def epoch(self, X, users, pos, negs, g_batches, gpr_batches, d_bsize):
        """users / pos: the epoch's order; negs: per pass (G's negatives, G''s negatives); g_batches: per step (users, nu bool, items);
        gpr_batches: per step (users, items).  Returns (d_losses, g_losses, gpr_losses)."""
        dl, gl, pl = [], [], []
        for ng, np_ in negs:
            for s in range(0, len(users), d_bsize):
                sl = slice(s, min(s + d_bsize, len(users)))
                dl.append(self.d_step(users[sl], pos[sl], ng[sl]))
                dl.append(self.d_step(users[sl], pos[sl], np_[sl]))
        for us, nu, it in g_batches:
            gl.append(self.g_step(0, us, X, nu, it))
        for us, it in gpr_batches:
            pl.append(self.g_step(1, us, X, None, it))
        return np.array(dl), np.array(gl), np.array(pl)


# -- |terms| bounds ------------------------------------------------------------------------------------------------------------------
def abs_d_bounds(ref, u, i, j):
    """ref: a float64 CAAERef.  Per element of P, Q and b the sum of |terms| of d_grads; the coefficient's own rounding enters through
    the logit's |terms| times sup sigmoid' = 0.25, as helpers_cfgan.abs_d_bounds carries its logit."""
    P, Q, b = (np.abs(a) for a in ref.p["D"])
    u, i, j = (np.asarray(a, dtype=np.int64) for a in (u, i, j))
    B = float(len(u))
    beta = abs(float(ref.beta))
    p0, q0, b0 = ref.p["D"]
    x = np.sum(p0[u] * (q0[i] - q0[j]), axis=1) + (b0[i] - b0[j])
    xa = np.sum(P[u] * (Q[i] + Q[j]), axis=1) + (b[i] + b[j])
    c = (np.exp(log_sigmoid(-x)) + 0.25 * xa) / B
    gP, gQ, gb = np.zeros_like(P), np.zeros_like(Q), np.zeros_like(b)
    np.add.at(gP, u, c[:, None] * (Q[i] + Q[j]) + beta * P[u])
    np.add.at(gQ, i, c[:, None] * P[u] + beta * Q[i])
    np.add.at(gQ, j, c[:, None] * P[u] + beta * Q[j])
    np.add.at(gb, i, c + beta * b[i])
    np.add.at(gb, j, c + beta * b[j])
    return [gP, gQ, gb]


def abs_g_bounds(ref, which, users, X, nu, items):
    """Per element of every tensor of G (or G') the sum of |terms| of g_grads.  Sigmoid: sup |act'| = 0.25, sup |act''| = 0.0962; the
    output r's own |terms| (RA) enter dr through the soft-max (|d s / d r| <= s) and the auto-encoder term."""
    key = "G" if which == 0 else "G_prime"
    P = [np.abs(a) for a in ref.p[key]]
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    x = np.asarray(X, dtype=np.float64)[users]
    m, n_s = items.shape
    h = ref.mlp(key, x)
    r = h[-1]
    s1, s2 = 0.25, 0.0962
    H, layers = np.abs(x), []
    for l in range(len(P) // 2):
        Z = H @ P[2 * l] + P[2 * l + 1]
        A = np.abs(h[l + 1]) + s1 * Z
        layers.append((H, Z))
        H = A
    RA = s1 * layers[-1][1]      # |terms| behind r
    lse = np.log(np.exp(r).sum(axis=1))
    sm = np.exp(r - lse[:, None])
    # a reward log sigmoid(y) with its own |terms|: |d log sigmoid / d y| <= 1 times the |terms| of y = <P_u, Q_j> + b_j -+ 1
    Pa, Qa, ba = (np.abs(a) for a in ref.p["D"])
    R = np.abs(ref.reward(which, users, items)) + np.einsum("bd,bsd->bs", Pa[users], Qa[items]) + ba[items] + 1.0
    lam = abs(float(ref.lmbda))
    pc = (lam if which == 0 else 1.0) / (m * n_s)
    hit = np.zeros_like(r)
    np.add.at(hit, (np.repeat(np.arange(m), n_s), items.ravel()), R.ravel())
    sumR = R.sum(axis=1)[:, None]
    DR = pc * (hit + sumR * sm * (1.0 + RA + (sm * RA).sum(axis=1)[:, None]))
    if which == 0:
        e = np.abs(x) + (np.asarray(nu, dtype=np.float64) if nu is not None else 0.0)
        DR = DR + 2.0 * abs(1.0 - lam) * (np.abs(r) + np.abs(x) + RA) * e * e
    beta = abs(float(ref.beta))
    g = [None] * len(P)
    DH = DR
    for l in reversed(range(len(P) // 2)):
        Hin, Z = layers[l]
        DZ = DH * (s1 + s2 * Z)
        g[2 * l] = Hin.T @ DZ + beta * P[2 * l]
        g[2 * l + 1] = DZ.sum(axis=0) + beta * P[2 * l + 1]
        DH = DZ @ P[2 * l].T
    return g


# -- the device samplers, restated -----------------------------------------------------------------------------------------------------
def base(seed, epoch, stream, step):
    return mix(mix(mix(mix(seed & _M64) ^ epoch) ^ stream) ^ step)


def u24(b, index):
    """the 24-bit uniform of every index, as the float32 in [0, 1) the device searches with"""
    w = mix_np(np.uint64(b) ^ np.asarray(index, dtype=np.uint64)) >> np.uint64(40)
    return w.astype(np.float32) * np.float32(2.0 ** -24)


def perm_index(b, n, t):
    half = 1
    while (1 << (2 * half)) < n:
        half += 1
    mask = (1 << half) - 1
    x = t
    while True:
        l, r = x >> half, x & mask
        for q in range(FEISTEL_ROUNDS):
            f = mix(b ^ (((q + 1) << 40) | r)) & mask
            l, r = r, l ^ f
        x = (l << half) | r
        if x < n:
            return x


def perm(seed, epoch, nnz):
    b = base(seed, epoch, STREAM_PERM, 0)
    return np.array([perm_index(b, nnz, t) for t in range(nnz)], dtype=np.int32)


def users(seed, epoch, which, step, m, U):
    b = base(seed, epoch, STREAM_USERS + which, step)
    if which == 0:
        return np.array([perm_index(b, U, t) for t in range(m)], dtype=np.int32)
    return np.array([((mix(b ^ t) >> 32) * U) >> 32 for t in range(m)], dtype=np.int32)


def cdf_draws(b, cdf_rows, rows):
    """draw of index t in cdf_rows[rows[t]]: np.searchsorted(row, a, 'left') clamped to I - 1"""
    a = u24(b, np.arange(len(rows)))
    last = cdf_rows.shape[1] - 1
    return np.array([min(int(np.searchsorted(cdf_rows[r], a[t], side="left")), last) for t, r in enumerate(rows)], dtype=np.int32)


def negatives(seed, epoch, pass_, which, cdf_rows, users_of_position):
    return cdf_draws(base(seed, epoch, STREAM_NEG + which, pass_), cdf_rows, users_of_position)


def policy_items(seed, epoch, which, step, cdf_rows, n_s):
    m = cdf_rows.shape[0]
    return cdf_draws(base(seed, epoch, STREAM_ITEMS + which, step), cdf_rows, np.repeat(np.arange(m), n_s)).reshape(m, n_s)
