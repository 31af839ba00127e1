"""Shared pieces of the CFGAN tests (not a conftest: imported by the modules that use them).

* CFGANRef: a numpy restatement of the model (generator, discriminator, both gradients, TF-1 Adam, an epoch), usable in float64 and
  float32: every array and scalar is held in `dtype`, so the float32 instance rounds where a float32 implementation would.
* abs_d_bounds / abs_g_bounds: per element, the fp64 sum of |terms| behind each gradient -- the same chains with every operand
  replaced by its absolute value, built the way helpers_grad._abs_dis_* builds DisGANMF's.
* sampler_masks: a uint64 restatement of the device sampler's key and selection rule.
* make_case: the small matrices the device tests share."""
import numpy as np
import scipy.sparse as sps

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
# (sup |act'|, sup |act''|) as in helpers_grad._ACT_SUP; relu' is 0 or 1 and piecewise constant (a pre-activation within rounding of 0
# would flip it: the random cases here have none)
ACT_SUP = {"linear": (1.0, 0.0), "tanh": (1.0, 0.77), "sigmoid": (0.25, 0.0962), "relu": (1.0, 0.0)}


def sigmoid(z):
    with np.errstate(over="ignore"):      # exp(-z) may overflow to inf for a very negative z: 1 / inf = 0 is the value wanted
        return z.dtype.type(1) / (z.dtype.type(1) + np.exp(-z))


def act(kind, z):
    if kind == "linear":
        return z
    if kind == "tanh":
        return np.tanh(z)
    if kind == "relu":
        return np.maximum(z, z.dtype.type(0))
    if kind == "sigmoid":
        return sigmoid(z)
    raise ValueError(kind)


def act_grad_out(kind, a):
    one = a.dtype.type(1)
    if kind == "linear":
        return np.ones_like(a)
    if kind == "tanh":
        return one - a * a
    if kind == "relu":
        return (a > 0).astype(a.dtype)
    return a * (one - a)


def sce(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits"""
    return np.maximum(x, x.dtype.type(0)) - x * x.dtype.type(z) + np.log1p(np.exp(-np.abs(x)))


class CFGANRef(object):
    def __init__(self, weights, d_act="linear", g_act="linear", d_lr=1e-3, g_lr=1e-3, d_reg=0.0, g_reg=0.0, zr_coefficient=0.0,
                 dtype=np.float64):
        """weights: {'D': [W0, b0, ..., Wo, bo], 'G': [...]} (ganmf_amd.CFGAN.init_weights' layout)"""
        self.dt = np.dtype(dtype).type
        self.p = {k: [np.array(a, dtype=dtype) for a in v] for k, v in weights.items()}
        self.m = {k: [np.zeros_like(a) for a in v] for k, v in self.p.items()}
        self.v = {k: [np.zeros_like(a) for a in v] for k, v in self.p.items()}
        self.pw = {k: [self.dt(BETA1), self.dt(BETA2)] for k in self.p}
        self.act = {"D": d_act, "G": g_act}
        self.lr = {"D": self.dt(d_lr), "G": self.dt(g_lr)}
        self.reg = {"D": self.dt(d_reg), "G": self.dt(g_reg)}
        self.coef = self.dt(zr_coefficient)
        self.L = {k: len(v) // 2 - 1 for k, v in self.p.items()}

    # ---- forward ------------------------------------------------------------------------------
    def _mlp(self, key, x):
        """hidden outputs [h_0 = x, h_1, ...] and the linear output"""
        h = [x]
        for l in range(self.L[key]):
            h.append(act(self.act[key], h[-1] @ self.p[key][2 * l] + self.p[key][2 * l + 1]))
        return h, h[-1] @ self.p[key][-2] + self.p[key][-1]

    def generator(self, c):
        return self._mlp("G", np.asarray(c, dtype=self.dt))

    def scores(self, c):
        return self.generator(c)[1]

    def _l2(self, key):
        s = self.dt(0)
        for a in self.p[key]:
            s = s + self.dt(0.5) * np.sum(a * a, dtype=self.dt)
        return s

    def _mlp_back(self, key, h, dout, want_params):
        """gradients of the layers (tensor order) and of the input, from d loss / d (linear output)"""
        P = self.p[key]
        g = [None] * len(P)
        if want_params:
            g[-2] = h[-1].T @ dout
            g[-1] = dout.sum(axis=0)
        dh = dout @ P[-2].T
        for l in reversed(range(self.L[key])):
            dz = dh * act_grad_out(self.act[key], h[l + 1])
            if want_params:
                g[2 * l] = h[l].T @ dz
                g[2 * l + 1] = dz.sum(axis=0)
            dh = dz @ P[2 * l].T
        return g, dh

    # ---- the two losses and their gradients --------------------------------------------------------
    def d_grads(self, c, M):
        c, M = np.asarray(c, dtype=self.dt), np.asarray(M, dtype=self.dt)
        B = self.dt(c.shape[0])
        gout = self.generator(c)[1] * M
        grads = [np.zeros_like(a) for a in self.p["D"]]
        loss = self.dt(0)
        for x, lab in ((c, 1.0), (gout, 0.0)):
            h, logit = self._mlp("D", np.concatenate([c, x], axis=1))
            loss = loss + np.sum(sce(logit[:, 0], lab), dtype=self.dt) / B
            dl = (sigmoid(logit) - self.dt(lab)) / B
            g, _ = self._mlp_back("D", h, dl, True)
            grads = [a + b for a, b in zip(grads, g)]
        loss = loss + self.reg["D"] * self._l2("D")
        grads = [g + self.reg["D"] * p for g, p in zip(grads, self.p["D"])]
        return loss, grads

    def g_grads(self, c, M, ZR):
        c, M, ZR = (np.asarray(a, dtype=self.dt) for a in (c, M, ZR))
        B = self.dt(c.shape[0])
        I = c.shape[1]
        hg, fake = self.generator(c)
        h, logit = self._mlp("D", np.concatenate([c, fake * M], axis=1))
        loss = np.sum(sce(logit[:, 0], 1.0), dtype=self.dt) / B + self.reg["G"] * self._l2("G")
        loss = loss + self.coef * (np.sum(fake * fake * ZR, dtype=self.dt) / B)
        dl = (sigmoid(logit) - self.dt(1)) / B
        _, dx = self._mlp_back("D", h, dl, False)
        dfake = M * dx[:, I:] + (self.dt(2) * self.coef / B) * fake * ZR
        grads, _ = self._mlp_back("G", hg, dfake, True)
        grads = [g + self.reg["G"] * p for g, p in zip(grads, self.p["G"])]
        return loss, grads

    # ---- TF-1 Adam ---------------------------------------------------------------------------------
    def _adam(self, key, grads):
        one = self.dt(1)
        b1p, b2p = self.pw[key]
        lr_t = self.lr[key] * np.sqrt(one - b2p) / (one - b1p)
        for i, g in enumerate(grads):
            self.m[key][i] = self.m[key][i] + (g - self.m[key][i]) * (one - self.dt(BETA1))
            self.v[key][i] = self.v[key][i] + (g * g - self.v[key][i]) * (one - self.dt(BETA2))
            self.p[key][i] = self.p[key][i] - (self.m[key][i] * lr_t) / (np.sqrt(self.v[key][i]) + self.dt(EPS))
        self.pw[key] = [b1p * self.dt(BETA1), b2p * self.dt(BETA2)]

    def step(self, kind, c, M, ZR=None):
        """one optimiser step; returns the loss at the pre-update parameters"""
        if kind == 0:
            loss, grads = self.d_grads(c, M)
            self._adam("D", grads)
        else:
            loss, grads = self.g_grads(c, M, ZR)
            self._adam("G", grads)
        return loss

    def epoch(self, C, PM, ZR, d_steps, g_steps, d_batch, g_batch):
        """C dense rows, PM / ZR 0-1 planes [rows, I]; returns (d_losses, g_losses)"""
        C = np.asarray(C, dtype=self.dt)
        M = C + np.asarray(PM, dtype=self.dt)
        ZR = np.asarray(ZR, dtype=self.dt)
        dl, gl = [], []
        for _ in range(d_steps):
            for s in range(0, C.shape[0], d_batch):
                dl.append(self.step(0, C[s:s + d_batch], M[s:s + d_batch]))
        for _ in range(g_steps):
            for s in range(0, C.shape[0], g_batch):
                gl.append(self.step(1, C[s:s + g_batch], M[s:s + g_batch], ZR[s:s + g_batch]))
        return np.array(dl), np.array(gl)


# -- |terms| bounds ------------------------------------------------------------------------------------------------------------------
def _abs_chain(ref, key, x, x_abs):
    """per hidden layer (H_in, Z, A) magnitudes and the magnitude of the linear output, for the input x with magnitudes x_abs"""
    P = [np.abs(a) for a in ref.p[key]]
    h, _ = ref._mlp(key, x)
    s1 = ACT_SUP[ref.act[key]][0]
    H = x_abs
    layers = []
    for l in range(ref.L[key]):
        Z = H @ P[2 * l] + P[2 * l + 1]
        A = Z if ref.act[key] == "linear" else np.abs(h[l + 1]) + s1 * Z
        layers.append((H, Z, A))
        H = A
    return layers, H @ P[-2] + P[-1]


def _abs_back(ref, key, layers, DOUT, g=None):
    P = [np.abs(a) for a in ref.p[key]]
    s1, s2 = ACT_SUP[ref.act[key]]
    if g is not None:
        g[-2] += layers[-1][2].T @ DOUT
        g[-1] += DOUT.sum(axis=0)
    DH = DOUT @ P[-2].T
    for l in reversed(range(ref.L[key])):
        H, Z, _ = layers[l]
        DZ = DH * (s1 + s2 * Z)
        if g is not None:
            g[2 * l] += H.T @ DZ
            g[2 * l + 1] += DZ.sum(axis=0)
        DH = DZ @ P[2 * l].T
    return DH


def abs_d_bounds(ref, c, M):
    """ref: a float64 CFGANRef.  Per element of every discriminator tensor, the sum of |terms| of d_grads."""
    c, M = np.asarray(c, np.float64), np.asarray(M, np.float64)
    B = c.shape[0]
    fake = ref.generator(c)[1]
    fake_abs = _abs_chain(ref, "G", c, np.abs(c))[1]
    g = [np.zeros_like(a) for a in ref.p["D"]]
    for x, x_abs, lab in ((c, np.abs(c), 1.0), (fake * M, fake_abs * np.abs(M), 0.0)):
        inp, inp_abs = np.concatenate([c, x], axis=1), np.concatenate([np.abs(c), x_abs], axis=1)
        layers, Lg = _abs_chain(ref, "D", inp, inp_abs)
        logit = ref._mlp("D", inp)[1]
        DL = (np.abs(1.0 / (1.0 + np.exp(-logit)) - lab) + 0.25 * Lg) / B
        _abs_back(ref, "D", layers, DL, g)
    return [a + abs(float(ref.reg["D"])) * np.abs(p) for a, p in zip(g, ref.p["D"])]


def abs_g_bounds(ref, c, M, ZR):
    c, M, ZR = (np.asarray(a, np.float64) for a in (c, M, ZR))
    B, I = c.shape
    fake = ref.generator(c)[1]
    glayers, fake_abs = _abs_chain(ref, "G", c, np.abs(c))
    inp, inp_abs = np.concatenate([c, fake * M], axis=1), np.concatenate([np.abs(c), fake_abs * np.abs(M)], axis=1)
    layers, Lg = _abs_chain(ref, "D", inp, inp_abs)
    logit = ref._mlp("D", inp)[1]
    DL = (np.abs(1.0 / (1.0 + np.exp(-logit)) - 1.0) + 0.25 * Lg) / B
    DX = _abs_back(ref, "D", layers, DL)
    dfake = np.abs(M) * DX[:, I:] + (2.0 * abs(float(ref.coef)) / B) * fake_abs * ZR
    g = [np.zeros_like(a) for a in ref.p["G"]]
    _abs_back(ref, "G", glayers, dfake, g)
    return [a + abs(float(ref.reg["G"])) * np.abs(p) for a, p in zip(g, ref.p["G"])]


# -- the device sampler, restated ------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def mix(z):
    """the splitmix64 output function on a Python int"""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def mix_np(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sampler_keys(seed, epoch, plane, row, cols):
    base = mix(mix(mix(seed & _M64) ^ epoch) ^ plane)
    ctr = np.uint64(base) ^ ((np.uint64(row) << np.uint64(32)) | np.asarray(cols, dtype=np.uint64))
    return (mix_np(ctr) >> np.uint64(32)).astype(np.uint32)


def sampler_row(seed, epoch, plane, row, eligible, k):
    """the k eligible columns with the smallest (key, column) pairs"""
    eligible = np.asarray(eligible, dtype=np.int64)
    keys = sampler_keys(seed, epoch, plane, row, eligible)
    order = np.lexsort((eligible, keys))
    return eligible[order[:k]]


def sampler_masks(urm, scheme, k_rows, seed, epoch):
    """(zr, pm) bool [rows, I] as ganmf_cfgan_draw_masks leaves them: plane 0 = ZR (schemes ZR, ZP), plane 1 = PM (PM, ZP)"""
    urm = sps.csr_matrix(urm)
    out = [np.zeros(urm.shape, dtype=bool), np.zeros(urm.shape, dtype=bool)]
    for plane, used in ((0, scheme in ("ZR", "ZP")), (1, scheme in ("PM", "ZP"))):
        if not used:
            continue
        for u in range(urm.shape[0]):
            prof = urm.indices[urm.indptr[u]:urm.indptr[u + 1]]
            free = np.setdiff1d(np.arange(urm.shape[1]), prof)
            k = min(int(k_rows[u]), len(free))
            out[plane][u, sampler_row(seed, epoch, plane, u, free, k)] = True
    return out[0], out[1]


# -- shared cases --------------------------------------------------------------------------------------------------------------------
def make_case(I, rows=65, seed=0):
    """`rows` x I float32 CSR with ratings 1..5 whose first rows have profiles of 0, 1, 63, 64, 65, I - 1 and I items (those that fit),
    the others random sizes"""
    rng = np.random.RandomState(seed)
    sizes = [s for s in (0, 1, 63, 64, 65, I - 1, I) if 0 <= s <= I]
    sizes += list(rng.randint(1, max(2, I // 3), size=rows - len(sizes)))
    dense = np.zeros((rows, I), dtype=np.float32)
    for r, s in enumerate(sizes[:rows]):
        cols = rng.choice(I, size=s, replace=False)
        dense[r, cols] = rng.randint(1, 6, size=s)
    m = sps.csr_matrix(dense)
    m.sort_indices()
    return m
