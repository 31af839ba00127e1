"""CPU controls of the row-by-row gradient rule of tests/test_gpu_grad_routes.py (no GPU): the float32 oracle, standing in for a
kernel, passes it, and each of the faults the rule is there to catch -- a gradient row off by 1e-3 of itself, a dropped split-K slab,
two batch rows swapped, a row_offset off by one in the float(uid) row, a bias gradient without its d_reg term -- fails it.  The last
test shows the blind spot that makes the rule necessary: Adam's first step hardly sees a constant scale of the gradient."""
import numpy as np
import pytest
import scipy.sparse as sps

from oracle.ganmf_oracle import _Adam, DisGANMFOracle, GANMFOracle
from tests.helpers_grad import _rowwise, allowed, d_bounds, g_bounds, row_ratio

U, N, K, E, B = 50, 120, 6, 24, 16
HP = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-2, recon_coefficient=0.3)


def _urm(rng):
    m = (rng.rand(U, N) < 0.08) * rng.randint(1, 6, (U, N))
    m[:, :5] = 0                        # items nobody rated
    return sps.csr_matrix(m.astype(np.float32))


def _case(kind, act="linear", layers=1):
    rng = np.random.RandomState({"ganmf": 1, "linear": 2, "tanh": 3, "sigmoid": 4}[kind if kind == "ganmf" else act])
    urm = _urm(rng)
    if kind == "ganmf":
        make = lambda dt: GANMFOracle(U, N, K, E, dtype=dt, seed=5, m=5.0, g_reg=0.0, **HP)
        extra = dict(be=rng.randn(E) * 0.1, bd=rng.randn(N) * 0.1)
    else:
        make = lambda dt: DisGANMFOracle(U, N, K, d_layers=layers, d_nodes=E, d_hidden_act=act, dtype=dt, seed=5, g_reg=0.0, **HP)
        extra = {"b%d" % l: rng.randn(E) * 0.1 for l in range(layers)}
        extra["bo"] = rng.randn(1) * 0.1
    o, o32 = make(np.float64), make(np.float32)
    if kind != "ganmf":
        o.p["W0"][0, :] *= 1.0 / U
        if act == "tanh":       # pre-activations in tanh's near-linear range (see test_gpu_grad_routes.py)
            for l in range(layers):
                o.p["W%d" % l] *= 0.3
    o.set_params(**extra)
    p0 = {n: v.astype(np.float32) for n, v in o.p.items()}
    o.set_params(**p0)
    o32.set_params(**p0)
    uids = rng.choice(U, B, replace=False)
    X = urm[uids].toarray().astype(np.float64)
    _, gd = o.d_grads(uids, X)
    _, gd32 = o32.d_grads(uids, X.astype(np.float32))
    _, gg = o.g_grads(uids, X)
    _, gg32 = o32.g_grads(uids, X.astype(np.float32))
    ref = dict(gd, **gg)
    got = dict(gd32, **gg32)
    bound = dict(d_bounds(o, uids, X), **g_bounds(o, uids, X))
    r32 = {n: row_ratio(got[n], ref[n], bound[n])[0] for n in ref}
    return o, uids, X, ref, got, bound, r32


def _check(got, ref, bound, r32, what):
    _rowwise(got, ref, bound, what, tol=allowed(r32))


GANMF = _case("ganmf")
DIS = {act: _case("dis", act, 2 if act == "tanh" else 1) for act in ("linear", "tanh", "sigmoid")}


@pytest.mark.parametrize("kind", ["ganmf", "linear", "tanh", "sigmoid"])
def test_float32_oracle_passes_the_rule(kind):
    """The float32 evaluation of the same arithmetic is within the rule on every tensor (and within 2e-5 outright: the bounds are
    not so tight that fp32 rounding alone fails them), and no bound is 0 where the gradient is not."""
    _, uids, _, ref, got, bound, r32 = GANMF if kind == "ganmf" else DIS[kind]
    for n in ref:
        _check(got[n], ref[n], bound[n], r32[n], (kind, n))
        assert r32[n] <= 2e-5, (kind, n, r32[n])
        assert np.all(bound[n] >= np.abs(ref[n]) * (1 - 1e-12)), (kind, n)      # a sum of |terms| bounds the sum
    rows_u = np.zeros(U, bool)
    rows_u[uids] = True
    assert np.all(bound["U"][~rows_u] == 0) and np.all(bound["U"][rows_u].max(axis=1) > 0)


def _fails(got, ref, bound, r32, what):
    with pytest.raises(AssertionError):
        _check(got, ref, bound, r32, what)


@pytest.mark.parametrize("scale", [1 + 1e-3, 1 - 1e-3])
def test_one_row_off_by_a_small_factor_fails(scale):
    """one gWe row -- of the item with the smallest bound -- scaled by 1 +- 1e-3.  (Not 1e-4: a row's largest |g| is 4-8 % of its
    largest |terms| bound here -- the cancellation of a sum of B e signed terms -- so at the 2e-5 floor of the rule a row is resolved
    to about 5e-4 of its own size; the float32 oracle itself is at 1e-8 of the bound.)"""
    _, _, _, ref, got, bound, r32 = GANMF
    i = int(np.argmin(bound["We"].max(axis=1)))
    bad = got["We"].astype(np.float64).copy()
    bad[i] *= scale
    _fails(bad, ref["We"], bound["We"], r32["We"], "We row %d" % i)


def test_dropped_split_k_slab_fails():
    """gWd summed without one quarter of the batch rows, real and generated (a split-K slab left out of the reduce)"""
    o, uids, X, ref, got, bound, r32 = GANMF
    F = o.generator(uids)
    Er, dr, Lr = o.autoencoder(X)
    Ef, df, Lf = o.autoencoder(F)
    active = o.m * Lr - Lf > 0
    s = 2.0 / (B * N)
    q = slice(3 * B // 4, B)
    slab = Er[q].T @ (((1.0 + (o.m if active else 0.0)) * s) * dr[q]) + Ef[q].T @ (((-1.0 if active else 0.0) * s) * df[q])
    _fails(ref["Wd"] - slab, ref["Wd"], bound["Wd"], r32["Wd"], "gWd without a slab")


def test_swapped_batch_rows_fail():
    """two batch rows of gU swapped"""
    _, uids, _, ref, got, bound, r32 = GANMF
    bad = got["U"].astype(np.float64).copy()
    bad[[uids[0], uids[1]]] = bad[[uids[1], uids[0]]]
    _fails(bad, ref["U"], bound["U"], r32["U"], "gU rows swapped")


@pytest.mark.parametrize("act", ["linear", "tanh", "sigmoid"])
def test_uid_row_off_by_one_fails(act):
    """the float(uid) row of gW0 formed with uid + 1 (a row_offset off by one): sum_b (uid_b + 1) dz_b = gW0[0] + sum_b dz_b"""
    o, _, _, ref, got, bound, r32 = DIS[act]
    bad = got["W0"].astype(np.float64).copy()
    bad[0] += ref["b0"] - float(o.d_reg) * o.p["b0"]
    _fails(bad, ref["W0"], bound["W0"], r32["W0"], (act, "uid + 1"))


@pytest.mark.parametrize("kind,name", [("ganmf", "be"), ("ganmf", "bd"), ("tanh", "b1"), ("sigmoid", "b0"), ("linear", "bo")])
def test_bias_without_d_reg_fails(kind, name):
    """a bias gradient without its d_reg term"""
    o, _, _, ref, got, bound, r32 = GANMF if kind == "ganmf" else DIS[kind]
    bad = got[name].astype(np.float64) - float(o.d_reg) * o.p[name]
    _fails(bad, ref[name], bound[name], r32[name], (kind, name, "no d_reg"))


def test_adam_first_step_is_blind_to_gradient_scale():
    """The blind spot: one TF-Adam step from zero moments on g and on 1.5 g gives parameters equal to within 1e-6 lr wherever
    |g| >= 0.11 (the update is lr g / (|g| + eps / sqrt(1 - b2)) ~ +-lr), and to within 1.1e-3 lr wherever |g| >= 1e-4 -- a kernel
    that forms the gradient 50 % too large leaves the parameters (and the losses of the next step) all but unchanged."""
    o = GANMF[0]
    g = GANMF[3]["We"]
    lr = 1e-3
    out = []
    for scale in (1.0, 1.5):
        opt = _Adam(lr, np.float64)
        p = o.p["We"].copy()
        opt.apply_dense("We", p, scale * g)
        out.append(p)
    d = np.abs(out[0] - out[1])
    a = np.abs(g)
    # |delta| = lr eps' (1/|g| - 1/(1.5 |g|)) / (1 + eps'/|g|)...  <= lr eps' / (3 |g|), eps' = eps / sqrt(1 - b2) = 3.2e-7
    assert np.all(d <= 1.1e-7 * lr / a + 1e-18)
    assert np.all(d[a >= 0.11] <= 1e-6 * lr) and np.all(d[a >= 1e-4] <= 1.1e-3 * lr)
    assert (a >= 0.11).any() and np.median(d / lr) <= 1e-4
    # ... while the rule sees it at once
    _fails(1.5 * g, g, GANMF[5]["We"], GANMF[6]["We"], "1.5 g")


def test_moment_bounds_initial_magnitude():
    """A warm start: |m0| and |v0| enter decayed by b1^T and b2^T; without them the bounds are those from zero moments."""
    from tests.helpers_grad import MomentBounds
    rng = np.random.RandomState(0)
    g = [rng.randn(3, 4) for _ in range(5)]
    b = [np.abs(rng.randn(3, 4)) for _ in range(5)]
    m0, v0 = rng.randn(3, 4), np.abs(rng.randn(3, 4))
    cold, cold2, warm = MomentBounds(), MomentBounds(None, None), MomentBounds({"w": m0}, {"w": v0})
    for gi, bi in zip(g, b):
        for mb in (cold, cold2, warm):
            mb.add("w", gi, bi)
    np.testing.assert_array_equal(cold.m["w"], cold2.m["w"])
    np.testing.assert_array_equal(cold.v["w"], cold2.v["w"])
    np.testing.assert_allclose(warm.m["w"] - cold.m["w"], np.abs(m0) * 0.9 ** 5, rtol=1e-9)
    np.testing.assert_allclose(warm.v["w"] - cold.v["w"], v0 * 0.999 ** 5, rtol=1e-9)


def test_set_state_loads_an_oracle():
    """set_state: fp32 values widened to the oracle's dtype and reshaped to its variables; powers in the order {D, D, G, G},
    formed by adam_powers_after as _Adam.finish forms them."""
    from tests.helpers_grad import adam_powers_after, set_state
    o = GANMFOracle(6, 5, 2, 3, dtype=np.float64)
    rng = np.random.RandomState(1)
    p = {n: rng.randn(*a.shape).astype(np.float32) for n, a in o.p.items()}
    m = {n: rng.randn(1, a.size).astype(np.float32) for n, a in o.p.items()}
    v = {n: np.abs(rng.randn(a.size)).astype(np.float32) for n, a in o.p.items()}
    opt = _Adam(1e-3, np.float32)
    for _ in range(7):
        opt.finish()
    assert adam_powers_after(7) == (opt.b1p, opt.b2p) and adam_powers_after(0) == (np.float32(0.9), np.float32(0.999))
    pw = adam_powers_after(7) + adam_powers_after(2)
    set_state(o, p, m, v, pw)
    for n in o.p:
        slots = (o.opt_d if n in o.D_NAMES else o.opt_g).slots[n]
        assert o.p[n].dtype == np.float64 and slots[0].shape == o.p[n].shape and slots[1].dtype == np.float64
        np.testing.assert_array_equal(o.p[n], p[n].astype(np.float64))
        np.testing.assert_array_equal(slots[0].ravel(), m[n].ravel().astype(np.float64))
        np.testing.assert_array_equal(slots[1].ravel(), v[n].ravel().astype(np.float64))
    assert (o.opt_d.b1p, o.opt_d.b2p, o.opt_g.b1p, o.opt_g.b2p) == tuple(np.float64(x) for x in pw)
