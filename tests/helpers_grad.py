"""Shared pieces of the gradient checks against the fp64 oracle (not a conftest: imported by the modules that use them).

* |terms| bounds: per element, the fp64 sum of |terms| behind each gradient of GANMFOracle / DisGANMFOracle.d_grads / g_grads -- the
  same chain with every operand replaced by its absolute value, what a rounding error of that element is proportional to.
* _rowwise / row_ratio / allowed: each row of a gradient is held to its own bound, not to the tensor's largest element (one wrong
  row of a rarely rated item, or of one user, must fail).
* grad_from_m: the gradient of one step read from SLOT_ADAM_M after a step from zero moments (m = (1 - beta1) g).
* plan_lines / forms: the kernel forms a run took, from the GANMF_DEBUG_PLAN lines and the class names of Engine.profile_read().
* adam_powers_after / set_state: a warm training state (parameters, both moments, the four beta powers) loaded into an oracle."""
import re

import numpy as np

from oracle.ganmf_oracle import BETA1, BETA2

# (sup |act'|, sup |act''|): the activation derivative at its supremum, and how far the rounding of z moves it
# (tanh'' <= 4 / (3 sqrt 3) = 0.770, sigmoid'' <= sqrt 3 / 18 = 0.0962)
_ACT_SUP = {"linear": (1.0, 0.0), "tanh": (1.0, 0.77), "sigmoid": (0.25, 0.0962)}


# -- |terms| bounds --------------------------------------------------------------------------------------------------------------
def _abs_d_bounds(o, uids, X):
    """Per element, the fp64 sum of |terms| behind each discriminator gradient (the GEMM chain encode -> decode -> dR -> dE -> gW
    with every operand replaced by its absolute value; hinge coefficients at their largest): what a rounding error of that element
    is proportional to."""
    p = {n: np.abs(v) for n, v in o.p.items()}
    N = X.shape[1]
    s = 2.0 / (X.shape[0] * N)
    g = {n: np.zeros_like(p[n]) for n in o.D_NAMES}
    Fa = p["U"][uids] @ p["V"].T
    for inp, c in ((np.abs(X), 1.0 + float(o.m)), (Fa, 1.0)):
        Ea = inp @ p["We"] + p["be"]
        dRa = (c * s) * (Ea @ p["Wd"] + p["bd"] + inp)
        g["Wd"] += Ea.T @ dRa
        g["bd"] += dRa.sum(axis=0)
        dEa = dRa @ p["Wd"].T
        g["We"] += inp.T @ dEa
        g["be"] += dEa.sum(axis=0)
    for n in o.D_NAMES:
        g[n] += abs(float(o.d_reg)) * p[n]
    return g


def _abs_g_bounds(o, uids, X):
    p = {n: np.abs(v) for n, v in o.p.items()}
    B, N = X.shape
    a = float(o.alpha)
    Ub = p["U"][uids]
    Fa = Ub @ p["V"].T
    Era = np.abs(X) @ p["We"] + p["be"]
    Efa = Fa @ p["We"] + p["be"]
    dRa = ((1.0 - a) * 2.0 / (B * N)) * (Efa @ p["Wd"] + p["bd"] + Fa)
    dEa = dRa @ p["Wd"].T + (a * 2.0 / (B * o.e)) * (Efa + Era)
    dFa = dEa @ p["We"].T + dRa
    gU = abs(float(o.g_reg)) * p["U"]
    gU[uids] += dFa @ p["V"]
    return {"U": gU, "V": dFa.T @ Ub + abs(float(o.g_reg)) * p["V"]}


def _dis_chain(o, uids, inp, inp_abs, p):
    """Per hidden layer (H_in, Z, A) magnitudes and the |logit| bound for one discriminator input."""
    cache, _, logit = o.discriminator(uids, inp)
    s1 = _ACT_SUP[o.act][0]
    uid_col = np.abs(np.asarray(uids, np.float64)).reshape(-1, 1)
    H = np.concatenate([uid_col, inp_abs], axis=1)
    out = []
    for l in range(o.L):
        Z = H @ p["W%d" % l] + p["b%d" % l]
        A = Z if o.act == "linear" else np.abs(np.asarray(cache[l][2], np.float64)) + s1 * Z
        out.append((H, Z, A))
        H = A
    Lg = (H @ p["Wo"] + p["bo"])[:, 0]
    return out, Lg, np.asarray(logit, np.float64)


def _dis_back(o, p, layers, DH, g=None):
    """|terms| of the backward chain from the feature-gradient magnitudes DH: dz = dh * act'(z) (act' at its supremum, plus the
    rounding of z reaching act' through sup |act''|), gW = H^T dz, gb = sum dz, dh_in = dz |W|^T.  Returns the layer-0 input
    magnitudes."""
    s1, s2 = _ACT_SUP[o.act]
    for l in reversed(range(o.L)):
        H, Z, _ = layers[l]
        DZ = DH * (s1 + s2 * Z)
        if g is not None:
            g["W%d" % l] += H.T @ DZ
            g["b%d" % l] += DZ.sum(axis=0)
        DH = DZ @ p["W%d" % l].T
    return DH


def _abs_dis_d_bounds(o, uids, X):
    """DisGANMFOracle.d_grads with every operand replaced by its absolute value: the float(uid) column (values up to U - 1) in the
    layer-0 input, activation derivatives at their supremum (1 for linear and tanh, 1/4 for sigmoid), and the rounding of the logit
    reaching dlogit through sigmoid' <= 1/4."""
    p = {n: np.abs(np.asarray(v, np.float64)) for n, v in o.p.items()}
    B = X.shape[0]
    g = {n: np.zeros_like(p[n]) for n in o.D_NAMES}
    Fa = p["U"][uids] @ p["V"].T
    F = o.p["U"][uids] @ o.p["V"].T
    for inp, inp_abs, lab in ((X, np.abs(X), 1.0), (F, Fa, 0.0)):
        layers, Lg, logit = _dis_chain(o, uids, inp, inp_abs, p)
        DL = (np.abs(1.0 / (1.0 + np.exp(-logit)) - lab) + 0.25 * Lg) / B
        g["Wo"] += layers[-1][2].T @ DL[:, None]
        g["bo"] += DL.sum(keepdims=True)
        _dis_back(o, p, layers, DL[:, None] @ p["Wo"].T, g)
    for n in o.D_NAMES:
        g[n] += abs(float(o.d_reg)) * p[n]
    return g


def _abs_dis_g_bounds(o, uids, X):
    """DisGANMFOracle.g_grads, the same way, with the feature-matching term alpha * 2 / (B e) (feat_f - feat_r) in dh."""
    p = {n: np.abs(np.asarray(v, np.float64)) for n, v in o.p.items()}
    B = X.shape[0]
    Ub = p["U"][uids]
    Fa = Ub @ p["V"].T
    F = o.p["U"][uids] @ o.p["V"].T
    layers_r, _, _ = _dis_chain(o, uids, X, np.abs(X), p)
    layers_f, Lg, logit = _dis_chain(o, uids, F, Fa, p)
    feat_r, feat_f = layers_r[-1][2], layers_f[-1][2]
    DL = (1.0 / (1.0 + np.exp(-logit)) + 0.25 * Lg) / B
    DH = DL[:, None] @ p["Wo"].T + (abs(float(o.alpha)) * 2.0 / feat_f.size) * (feat_f + feat_r)
    dF = _dis_back(o, p, layers_f, DH)[:, 1:]
    gU = abs(float(o.g_reg)) * p["U"]
    gU[uids] += dF @ p["V"]
    return {"U": gU, "V": dF.T @ Ub + abs(float(o.g_reg)) * p["V"]}


def d_bounds(o, uids, X):
    return _abs_d_bounds(o, uids, X) if hasattr(o, "m") else _abs_dis_d_bounds(o, uids, X)


def g_bounds(o, uids, X):
    return _abs_g_bounds(o, uids, X) if hasattr(o, "m") else _abs_dis_g_bounds(o, uids, X)


# -- the row-by-row rule ---------------------------------------------------------------------------------------------------------
def _rows(got, ref, bound):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    ref = np.asarray(ref, np.float64)
    bound = np.asarray(bound, np.float64)
    if got.ndim == 1:      # a bias vector: every element is its own row
        got, ref, bound = got[:, None], ref[:, None], bound[:, None]
    return np.abs(got - ref).max(axis=1), bound.max(axis=1)


def row_ratio(got, ref, bound):
    """(largest row ratio max|got - ref| / max bound over the rows whose bound is not 0, indices of bound-0 rows that differ)"""
    d, b = _rows(got, ref, bound)
    zero = b == 0
    r = d[~zero] / b[~zero]
    return (float(r.max()) if r.size else 0.0), np.flatnonzero(zero & (d != 0))


def _rowwise(got, ref, bound, what, tol=2e-5):
    """max |got - ref| of every row over the largest bound of that row; a row whose bound is 0 must be exactly 0."""
    d, b = _rows(got, ref, bound)
    zero = b == 0
    assert np.all(d[zero] == 0), (what, np.flatnonzero(zero & (d != 0))[:8])
    r = d[~zero] / b[~zero]
    assert r.size == 0 or r.max() <= tol, (what, "row", int(np.flatnonzero(~zero)[np.argmax(r)]), float(r.max()))


def allowed(r32):
    """One rule for every route: a row ratio of at most max(2e-5, 2 x the float32 oracle's ratio on that tensor), never above 1e-4."""
    return min(1e-4, max(2e-5, 2.0 * r32))


# -- reading the gradient and composing the epoch bounds -------------------------------------------------------------------------
ONE_MINUS_B1 = np.float64(np.float32(1.0) - np.float32(BETA1))


def grad_from_m(m):
    """the gradient of one step from zero moments: SLOT_ADAM_M = (1 - beta1) g, divided as the fp32 step formed (1 - beta1)"""
    return np.asarray(m, np.float64) / ONE_MINUS_B1


class MomentBounds:
    """|terms| bounds of the Adam moments after T updates, composed from the per-step gradient bounds B_t:
    m: sum_t (1 - b1) b1^(T - t) B_t;   v: sum_t (1 - b2) b2^(T - t) 2 |g_t| B_t.
    m0 / v0 (name -> array, a warm start): the magnitudes of the initial moments enter as |m0| b1^T and |v0| b2^T, decayed like
    every term behind them; without them the bounds are those of a start from zero moments."""

    def __init__(self, m0=None, v0=None):
        self.m = {n: np.abs(np.asarray(a, np.float64)) for n, a in (m0 or {}).items()}
        self.v = {n: np.abs(np.asarray(a, np.float64)) for n, a in (v0 or {}).items()}

    def add(self, name, g, bound):
        g, bound = np.abs(np.asarray(g, np.float64)), np.asarray(bound, np.float64)
        m = self.m.get(name, 0.0)
        v = self.v.get(name, 0.0)
        self.m[name] = BETA1 * m + (1.0 - BETA1) * bound
        self.v[name] = BETA2 * v + (1.0 - BETA2) * 2.0 * g * bound


# -- a warm training state -------------------------------------------------------------------------------------------------------
def adam_powers_after(t):
    """(beta1_power, beta2_power) after t optimizer steps, formed in fp32 by repeated multiplication as _Adam.finish forms them"""
    b1, b2 = np.float32(BETA1), np.float32(BETA2)
    p1, p2 = b1, b2
    for _ in range(t):
        p1, p2 = np.float32(p1 * b1), np.float32(p2 * b2)
    return p1, p2


def set_state(o, params, m, v, powers):
    """Loads fp32 parameters, Adam moments (name -> array, any shape of the right size) and powers = (b1p_D, b2p_D, b1p_G, b2p_G)
    into an oracle, widened to its dtype: the _Adam attributes it already has (slots[name] = (m, v), b1p, b2p)."""
    o.set_params(**{n: np.asarray(a).reshape(o.p[n].shape) for n, a in params.items()})
    for opt, names, (b1p, b2p) in ((o.opt_d, o.D_NAMES, powers[:2]), (o.opt_g, o.G_NAMES, powers[2:])):
        for n in names:
            opt.slots[n] = tuple(np.array(np.asarray(a).reshape(o.p[n].shape), dtype=o.dtype) for a in (m[n], v[n]))
        opt.b1p, opt.b2p = opt.dt(b1p), opt.dt(b2p)


# -- route probe -----------------------------------------------------------------------------------------------------------------
_PLAN = re.compile(r"\[ganmf plan\] (.+?)\s+M=(\d+) N=(\d+) K=(\d+) batch=(\d+) -> tile (\d+) ring (\d+) kg (\d+) nsplit (\d+) "
                   r"\(kps \d+\) mfma (\w+) wgs \d+ est [\d.]+ us(.*)$")

# class names of lib/base.inc kTagName -> form (Engine.profile_read() returns them cut to PROF_NAME - 1 characters)
PROF_NAME = 48
CLASS_FORMS = {
    "gemm_generator[B,k]x[N,k]^T + CSR rows (one launch)": "front",
    "gemm_gWd[2B,e]^Tx[2B,N] + reduce_dE (one launch)": "gWd+reduce_dE",
    "gemm_gUb[B,N]x[N,k] + gemm_gV[B,N]^Tx[B,k] (one launch)": "gUb+gV pair",
    "gemm_dE[2B,N]x[e,N]^T + d_coef (one launch)": "dE+d_coef",
    "gemm_gWd + gemm_gWe, fused Adam (one launch)": "gWd+gWe fused Adam",
    "gemm_gWd[2B,e]^Tx[2B,N]": "gWd stand-alone",
    "d_coef+scale": "d_coef stand-alone",
}
_CLASS_FORMS = {k[:PROF_NAME - 1]: v for k, v in CLASS_FORMS.items()}


def plan_lines(text):
    """the [ganmf plan] lines of a GANMF_DEBUG_PLAN run as dicts"""
    out = []
    for line in text.splitlines():
        mt = _PLAN.search(line)
        if mt:
            tag, M, N, K, batch, tile, ring, kg, nsplit, mode, rest = mt.groups()
            out.append(dict(tag=tag.strip(), M=int(M), N=int(N), K=int(K), batch=int(batch), tile=int(tile), ring=int(ring),
                            kg=int(kg), nsplit=int(nsplit), mode=mode, rest=rest.strip()))
    return out


_URM_PLAN = re.compile(r"\[ganmf urm\] set_urm_csr .*-> sparse_g (\d) sparse_d (\d)")


def urm_paths(text):
    """(sparse_g, sparse_d) of every URM upload of a GANMF_DEBUG_PLAN run"""
    return [(int(a), int(b)) for a, b in _URM_PLAN.findall(text)]


def forms(plans, classes):
    """The set of forms a run took: plan-line suffixes, the arithmetic of each plan, split-K with the stand-alone reduce or in
    the launch, the decode as one 2B-row product (merged) or two batches, gV on the staged split-bf16 kernel, and the one-launch
    (or stand-alone) classes that ran."""
    seen = set()
    two_b = {p["M"] for p in plans if p["tag"].startswith(("gemm_encode", "gemm_dis_layer_fwd"))}      # 2B: real and generated rows
    for p in plans:
        r = p["rest"]
        if "(skinny-K stream)" in r:
            seen.add("skinny-K")
        elif "(skinny-N stream)" in r:
            seen.add("skinny-N")
        elif "(64 x 32 tiles" in r:
            seen.add("64x32")
        if p["mode"] == "bf16x3" and p["kg"] == 4:
            seen.add("bf16x3 kg4")
        if p["mode"] == "bf16x3" and p["tile"] == 128:
            seen.add("bf16x3 tile128")
        if p["mode"] == "f32" and p["kg"] == 1:
            seen.add("f32 kg1")
        if p["nsplit"] > 1:
            seen.add("split-K in-launch" if "(in-launch reduce)" in r else "split-K reduce")
        if "one launch with the" in r:
            seen.add("front")
        if p["tag"].startswith("gemm_decode") and p["batch"] == 2:
            seen.add("decode two-batch")
        if p["tag"].startswith("gemm_decode") and p["batch"] == 1 and p["M"] in two_b:
            seen.add("decode merged")
        if p["tag"].startswith("gemm_gV") and p["mode"] == "bf16x3" and p["tile"] == 64 and p["ring"] == 2:
            seen.add("gV staged")
    for c in classes:
        if c[:PROF_NAME - 1] in _CLASS_FORMS:
            seen.add(_CLASS_FORMS[c[:PROF_NAME - 1]])
    return seen
