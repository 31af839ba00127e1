"""CAAE on the host: the numpy restatement's gradients against torch.autograd in float64 for all three losses, the host initialisation,
the fit() parameter list, the host replay of the reference's draws against a straight-line restatement of CAAE.py:220-337, and the
restatement of the device samplers."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.CAAE import CAAE, init_weights, nu_size, policy_draws, random_choice_numpy, run_epoch_numpy
from ganmf_amd.CFGAN import non_interactions
from tests import helpers_caae as HC


def _case(seed=3, U=9, I=13, k=5, gl=2, gu=4):
    rng = np.random.RandomState(seed)
    X = (rng.rand(U, I) < 0.35) * rng.randint(1, 6, size=(U, I)).astype(np.float64)
    w = init_weights(seed, U, I, k, gl, gu)
    w = {key: [a.astype(np.float64) * 3 for a in v] for key, v in w.items()}
    for key in ("G", "G_prime"):
        for n in range(1, len(w[key]), 2):
            w[key][n] = rng.uniform(-0.5, 0.5, size=w[key][n].shape)
    return rng, X, w


def _torch_params(w):
    import torch
    torch.set_default_dtype(torch.float64)
    return {key: [torch.tensor(a, requires_grad=True) for a in v] for key, v in w.items()}


def test_d_gradients_match_autograd():
    torch = pytest.importorskip("torch")
    rng, X, w = _case()
    beta = 0.03
    u = np.array([2, 2, 5, 0, 2, 8, 5])      # duplicate users
    i = np.array([1, 4, 4, 7, 1, 3, 12])     # duplicate positives; item 4 is positive here ...
    j = np.array([4, 6, 9, 7, 0, 3, 1])      # ... and negative here; triples 3 and 5 have i == j; item 1 on both sides
    ref = HC.CAAERef(w, beta=beta)
    loss, grads = ref.d_grads(u, i, j)
    T = _torch_params(w)
    P, Q, b = T["D"]
    pu, qi, qj, bi, bj = P[u], Q[i], Q[j], b[i], b[j]
    x = (pu * (qi - qj)).sum(1) + (bi - bj)
    tl = -torch.log(torch.sigmoid(x)).mean() + beta * 0.5 * ((pu ** 2).sum() + (qi ** 2).sum() + (qj ** 2).sum() + (bi ** 2).sum()
                                                           + (bj ** 2).sum())
    tg = torch.autograd.grad(tl, T["D"])
    assert abs(loss - tl.item()) <= 1e-10 * abs(tl.item())
    for got, want in zip(grads, tg):
        assert np.abs(got - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max()


@pytest.mark.parametrize("which", [0, 1])
def test_generator_gradients_match_autograd(which):
    torch = pytest.importorskip("torch")
    rng, X, w = _case()
    lmbda, beta = 0.3, 0.02
    U, I = X.shape
    users = np.array([4, 0, 7, 4]) if which == 1 else np.array([4, 0, 7, 2])      # G' batches repeat users
    items = rng.randint(0, I, size=(4, 6))
    items[1, 3] = items[1, 0]                # a policy row that draws the same item twice
    nu = (rng.rand(4, I) < 0.4) & (X[users] == 0)
    key = "G" if which == 0 else "G_prime"
    ref = HC.CAAERef(w, lmbda=lmbda, beta=beta)
    loss, grads = ref.g_grads(which, users, X, nu if which == 0 else None, items)
    T = _torch_params(w)
    P, Q, b = (t.detach() for t in T["D"])
    x = torch.tensor(X[users])
    h = x
    for l in range(len(T[key]) // 2):
        h = torch.sigmoid(h @ T[key][2 * l] + T[key][2 * l + 1])
    it = torch.tensor(items)
    logit = (P[users][:, None, :] * Q[it]).sum(2) + b[it]
    reward = torch.log(torch.sigmoid(logit - 1)) if which == 0 else torch.log(torch.sigmoid(1 - logit))
    prob = torch.gather(torch.softmax(h, dim=1), 1, it)
    l2 = sum(0.5 * (p * p).sum() for p in T[key])
    if which == 0:
        e = x + torch.tensor(nu.astype(np.float64))
        tl = -lmbda * (torch.log(prob) * reward).mean() + (1 - lmbda) * (((h - x) * e) ** 2).sum() + beta * l2
    else:
        tl = -(torch.log(prob) * reward).mean() + beta * l2
    tg = torch.autograd.grad(tl, T[key])
    assert abs(loss - tl.item()) <= 1e-10 * abs(tl.item())
    for got, want in zip(grads, tg):
        assert got.shape == want.shape
        assert np.abs(got - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max()


def test_sgd_steps_and_epoch_apply_the_gradients():
    rng, X, w = _case()
    ref = HC.CAAERef(w, lmbda=0.3, beta=0.02, lr=0.1)
    _, g = HC.CAAERef(w, lmbda=0.3, beta=0.02).d_grads([1, 2], [3, 4], [5, 6])
    ref.d_step([1, 2], [3, 4], [5, 6])
    for p, p0, gr in zip(ref.p["D"], w["D"], g):
        assert np.array_equal(p, p0 - 0.1 * gr)
    f32 = HC.CAAERef(w, dtype=np.float32)
    loss, grads = f32.g_grads(0, [0, 1], X, np.zeros((2, X.shape[1]), bool), np.array([[1, 2], [3, 3]]))
    assert loss.dtype == np.float32 and all(a.dtype == np.float32 for a in grads)


def test_init_weights_shapes_limits_and_order():
    U, I, k, gl, gu = 11, 17, 3, 2, 5
    w = init_weights(7, U, I, k, gl, gu)
    rng = np.random.RandomState(7)

    def glorot(a, b):
        s = np.sqrt(6.0 / (a + b))
        return rng.uniform(-s, s, size=(a, b)).astype(np.float32)
    want = {"D": [glorot(U, k), glorot(I, k), rng.uniform(-np.sqrt(3.0 / I), np.sqrt(3.0 / I), size=I).astype(np.float32)]}
    for key in ("G", "G_prime"):      # dense biases are zero and draw nothing
        want[key] = [glorot(I, gu), np.zeros(gu, np.float32), glorot(gu, gu), np.zeros(gu, np.float32), glorot(gu, I),
                     np.zeros(I, np.float32)]
    assert list(w) == ["D", "G", "G_prime"]
    for key in want:
        assert len(w[key]) == len(want[key])
        for a, b in zip(w[key], want[key]):
            assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert np.abs(w["D"][2]).max() <= np.sqrt(3.0 / I) and np.abs(w["D"][0]).max() <= np.sqrt(6.0 / (U + k))
    assert w["G"][0].tobytes() != w["G_prime"][0].tobytes()


def test_fit_parameter_list_is_the_references():
    want = [("epochs", 300), ("d_steps", 1), ("g_steps", 1), ("gpr_steps", 1), ("g_layers", 1), ("g_units", 20), ("gpr_layers", 1),
            ("gpr_units", 20), ("num_factors", 10), ("d_bsize", 1024), ("m_batch", 32), ("lmbda", 0.5), ("beta", 1e-4), ("lr", 1e-4),
            ("S", 0.3), ("allow_worse", None), ("freq", None), ("after", 0), ("metrics", ["MAP"]), ("sample_every", None),
            ("validation_evaluator", None), ("validation_set", None)]
    fit = inspect.signature(CAAE.fit)
    assert [(n, p.default) for n, p in list(fit.parameters.items())[1:]] == want
    init = inspect.signature(CAAE.__init__)
    assert [(n, p.default) for n, p in list(init.parameters.items())[2:]] == [("verbose", False), ("mode", "user"), ("seed", 1234),
                                                                               ("is_experiment", False), ("device", 0),
                                                                               ("sampler", "device")]


def test_sizes_that_come_from_the_data():
    assert nu_size(10, 0.3) == 3 and nu_size(10, 0.7) == 7 and nu_size(100, 0.29) == 28      # a Python double, not a C float
    assert nu_size(0, 0.3) == 0
    urm = sps.csr_matrix(np.triu(np.ones((5, 7))))      # profile lengths 7, 6, 5, 4, 3: median 5
    assert policy_draws(urm) == 10
    m = CAAE(urm, mode="item", is_experiment=True)
    assert m.URM_train.shape == (5, 7) and (m.num_users, m.num_items) == (5, 7) and m.given_mode == "item" and m.mode == "user"
    with pytest.raises(ValueError, match="sampler"):
        CAAE(urm, sampler="tf", is_experiment=True)
    with pytest.raises(ValueError, match="m_batch"):
        m.fit(epochs=1, m_batch=6)
    with pytest.raises(ValueError, match="g_layers"):
        m.fit(epochs=1, g_layers=0)
    with pytest.raises(RuntimeError):
        m._compute_item_score(np.arange(2))


class _Backend(object):
    """arithmetic stand-in: fixed CDFs, every call recorded"""

    def __init__(self, U, I, seed):
        rng = np.random.RandomState(seed)
        self.cdfs = []
        for _ in range(2):
            p = rng.rand(U, I) + 0.05
            self.cdfs.append(np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1).astype(np.float32))
        self.calls = []

    def cdf_all(self, which):
        return self.cdfs[which]

    def cdf_rows(self, which, users):
        return self.cdfs[1 - which][np.asarray(users)]      # (another array than cdf_all's: the two must not be confused)

    def d_step(self, u, i, j):
        self.calls.append(("d", np.array(u), np.array(i), np.array(j)))
        return 0.0

    def g_step(self, which, users, nu, items):
        self.calls.append(("g", which, np.array(users), None if nu is None else np.array(nu), np.array(items)))
        return 0.0


def _search(row, a):
    lo, hi = 0, len(row)
    while lo < hi:      # cython_utils.pyx:166-181
        mid = (lo + hi) // 2
        if row[mid] < a:
            lo = mid + 1
        else:
            hi = mid
    return min(lo, len(row) - 1)


def test_numpy_sampler_consumes_the_stream_in_the_references_order():
    U, I, S, m_batch, d_bsize = 9, 14, 0.3, 4, 16
    rng = np.random.RandomState(2)
    d = (rng.rand(U, I) < 0.3).astype(np.float32)
    d[1] = 1          # full profile: no non-interaction
    d[2] = 0          # empty profile
    urm = sps.csr_matrix(d)
    n_s = policy_draws(urm)
    free = non_interactions(urm)
    users_of = np.repeat(np.arange(U, dtype=np.int32), np.diff(urm.indptr))
    order = np.arange(urm.nnz)
    be = _Backend(U, I, 5)
    np.random.seed(11)
    for _ in range(2):      # two epochs: the order stays shuffled from one to the next
        run_epoch_numpy(be, order, users_of, urm.indices, free, U, I, 2, 2, 1, d_bsize, m_batch, n_s, S)
    got = be.calls

    # CAAE.py:193-337, straight line, on the same stream
    np.random.seed(11)
    want = []
    all_interactions = [(u, i) for u in range(U) for i in urm.indices[urm.indptr[u]:urm.indptr[u + 1]]]
    cdf_g, cdf_p = be.cdfs
    prob_p = np.diff(cdf_p.astype(np.float64), axis=1, prepend=0.0)
    for _ in range(2):
        np.random.shuffle(all_interactions)
        us, pos = (np.array(a) for a in zip(*all_interactions))
        for _ in range(2):
            samples = np.random.random(2 * len(us)).astype(np.float32)
            g_neg = np.array([_search(cdf_g[u], samples[t]) for t, u in enumerate(us)])
            p_neg = np.array([_search(cdf_p[u], samples[len(us) + t]) for t, u in enumerate(us)])
            for s in range(0, len(us), d_bsize):
                want.append(("d", us[s:s + d_bsize], pos[s:s + d_bsize], g_neg[s:s + d_bsize]))
                want.append(("d", us[s:s + d_bsize], pos[s:s + d_bsize], p_neg[s:s + d_bsize]))
        for _ in range(2):
            uids = np.random.choice(np.arange(U, dtype=np.int32), size=m_batch, replace=False)
            nu = np.zeros((m_batch, I), dtype=bool)
            for r, u in enumerate(uids):
                if int(len(free[u]) * S):
                    p = prob_p[u, free[u]]
                    nu[r, np.random.choice(free[u], size=int(len(free[u]) * S), p=p / p.sum(), replace=False)] = True
            samples = np.random.random(m_batch * n_s).astype(np.float32)
            cdf = be.cdfs[1][uids]
            items = np.array([_search(cdf[t // n_s], samples[t]) for t in range(m_batch * n_s)]).reshape(m_batch, n_s)
            want.append(("g", 0, uids, nu, items))
        uids = np.random.choice(np.arange(U, dtype=np.int32), size=m_batch)
        samples = np.random.random(m_batch * n_s).astype(np.float32)
        cdf = be.cdfs[0][uids]
        items = np.array([_search(cdf[t // n_s], samples[t]) for t in range(m_batch * n_s)]).reshape(m_batch, n_s)
        want.append(("g", 1, uids, None, items))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert (x is None and y is None) or np.array_equal(x, y), (a[0], x, y)
    assert np.random.random() == _next_after(11, be, urm, free, d_bsize, m_batch, n_s, S)


def _next_after(seed, be, urm, free, d_bsize, m_batch, n_s, S):
    """the stream's next value after the helper's two epochs, run again from the seed: the helper consumed nothing else"""
    np.random.seed(seed)
    order = np.arange(urm.nnz)
    users_of = np.repeat(np.arange(urm.shape[0], dtype=np.int32), np.diff(urm.indptr))
    for _ in range(2):
        run_epoch_numpy(_Backend(urm.shape[0], urm.shape[1], 5), order, users_of, urm.indices, free, urm.shape[0], urm.shape[1], 2, 2, 1,
                        d_bsize, m_batch, n_s, S)
    return np.random.random()


def test_random_choice_numpy_is_the_cython_routine():
    rng = np.random.RandomState(0)
    p = rng.rand(5, 8)
    cdf = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1).astype(np.float32)
    cdf[:, -1] = 0.999      # a sample above the last value clamps to I - 1
    np.random.seed(3)
    got = random_choice_numpy(cdf, size=4)
    np.random.seed(3)
    s = np.random.random(20).astype(np.float32)
    assert np.array_equal(got, [_search(cdf[t // 4], s[t]) for t in range(20)])
    rows = np.array([4, 0, 0, 2], dtype=np.int32)
    np.random.seed(4)
    a, b = random_choice_numpy(cdf, cdf[::-1].copy(), custom_ordered_rows=rows)
    np.random.seed(4)
    s = np.random.random(8).astype(np.float32)
    assert np.array_equal(a, [_search(cdf[r], s[t]) for t, r in enumerate(rows)])
    assert np.array_equal(b, [_search(cdf[::-1][r], s[4 + t]) for t, r in enumerate(rows)])


def test_sampler_restatement():
    from tests.helpers_cfgan import mix
    b = HC.base(1, 2, 3, 4)
    assert b == mix(mix(mix(mix(1) ^ 2) ^ 3) ^ 4)
    assert float(HC.u24(b, [5])[0]) == (mix(b ^ 5) >> 40) / 2.0 ** 24
    for n in (1, 2, 5, 16, 17, 1000):      # a bijection of [0, n) at every size, a different one per key
        p = np.array([HC.perm_index(b, n, t) for t in range(n)])
        assert np.array_equal(np.sort(p), np.arange(n))
    assert not np.array_equal(HC.perm(1, 2, 1000), HC.perm(1, 3, 1000))
    g, gp = HC.users(1, 2, 0, 0, 32, 65), HC.users(1, 2, 1, 0, 32, 65)
    assert len(set(g.tolist())) == 32 and g.max() < 65 and gp.max() < 65 and not np.array_equal(g, gp)
    cdf = np.array([[0.25, 0.5, 0.5, 1.0], [0.0, 0.0, 0.5, 0.999]], dtype=np.float32)
    d = HC.cdf_draws(b, cdf, np.zeros(2000, dtype=int))
    assert set(d.tolist()) == {0, 1, 3}      # an item of probability 0 is never drawn
    assert abs((d == 3).mean() - 0.5) < 0.06
    assert HC.cdf_draws(b, cdf, np.ones(2000, dtype=int)).max() == 3      # above the last value: clamped
