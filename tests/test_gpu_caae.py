"""CAAE on the device: the CDF rows against float64, the samplers against their uint64 restatement, the weighted subset Nu against its
sizes, against numpy's own choice(p=, replace=False) and against planes recorded on the device, one D-step and one G / G' step per row against the float64 restatement, the
one-call epoch against its own recorded draws fed step by step and against float64, and the class (fit with both samplers, scoring,
device evaluation, early stopping, the Saver bundle, the refusals).

Shapes: 65 rows, I = 64 / 70 / 400 (and 5000 for the CDF rows: a second 4096-column tile), profiles of 0, 1, 63, 64, 65, I - 1 and I
items among the first rows (helpers_cfgan.make_case): the row with I items has no non-interaction, the row with 0 an empty profile."""
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_caae as HC
from tests import helpers_cfgan as H
from tests.helpers_grad import _rows, allowed

pytestmark = pytest.mark.gpu

ROWS = 65
DIS_FACTOR, DIS_FLOOR = 4.0, 5e-5      # test_gpu_cfgan.py / test_gpu_trajectory.py
ULP = 2.0 ** -23


def _engine(urm, k=4, g_units=4, g_layers=1, d_bsize=64, m_batch=32, n_s=None, lmbda=0.5, beta=1e-4, lr=1e-3, seed=0, S=0.3,
            k_rows=None):
    from ganmf_amd import _lib as L
    from ganmf_amd.CAAE import nu_size, policy_draws
    from ganmf_amd.engine import Engine
    eng = Engine(urm.shape[0], urm.shape[1], k, 1, 1, model=L.MODEL_CAAE)
    eng.set_urm(urm)
    if k_rows is None:
        k_rows = [nu_size(urm.shape[1] - int(n), S) for n in np.diff(urm.indptr)]
    eng.caae_init(g_units, g_layers, d_bsize, m_batch, policy_draws(urm) if n_s is None else n_s, lmbda, beta, lr, seed, k_rows)
    return eng


def _tids(gl):
    from ganmf_amd import _lib as L
    return {"D": [L.T_USER_EMB, L.T_ITEM_EMB, L.T_CAAE_ITEM_BIAS], "G": [L.T_CAAE_G0 + i for i in range(2 * gl + 2)],
            "G_prime": [L.T_CAAE_GPR0 + i for i in range(2 * gl + 2)]}


def _weights(urm, k, gl, gu, seed=1, scale=1.0):
    from ganmf_amd.CAAE import init_weights
    w = init_weights(seed, urm.shape[0], urm.shape[1], k, gl, gu)
    rng = np.random.RandomState(seed + 100)      # dense biases start at zero: give them values so that their chains are exercised
    for key in ("G", "G_prime"):
        for i in range(1, len(w[key]), 2):
            w[key][i] = rng.uniform(-0.5, 0.5, size=w[key][i].shape).astype(np.float32)
    return {key: [(a * scale).astype(np.float32) for a in v] for key, v in w.items()}


def _set_state(eng, w, gl):
    for key, ids in _tids(gl).items():
        for tid, a in zip(ids, w[key]):
            eng.set_tensor(tid, a)


def _get(eng, key, gl, like):
    return [eng.get_tensor(t).reshape(a.shape) for t, a in zip(_tids(gl)[key], like[key])]


def _ratio(got, ref, bound, theta):
    """largest row ratio of a gradient read as theta_before - theta_after at lr = 1: that difference is the gradient to within one ulp
    of theta (the rounding of the stored theta_after), so a row's difference is first reduced by max |theta| * 2^-23 of the row"""
    d, b = _rows(got, ref, bound)
    t = np.abs(np.asarray(theta, np.float64).reshape(np.shape(ref)))
    t = (t[:, None] if t.ndim == 1 else t).max(axis=1)
    d = np.maximum(d - t * ULP, 0.0)
    zero = b == 0
    r = d[~zero] / b[~zero]
    return (float(r.max()) if r.size else 0.0), np.flatnonzero(zero & (d != 0))


# ---- CDF rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [64, 70, 400, 5000])
def test_cdf_rows_against_float64(I):
    urm = H.make_case(I)
    w = _weights(urm, 4, 2, 6, scale=3.0)
    eng = _engine(urm, g_units=6, g_layers=2)
    _set_state(eng, w, 2)
    ref = HC.CAAERef(w)
    X = urm.toarray()
    tol = (I + 8) * 2.0 ** -24
    worst = 0.0
    for which, key in ((0, "G"), (1, "G_prime")):
        want, lse64 = ref.cdf(key, X)
        sub = np.array([5, 0, 64, 6, 5])
        for got, lse, rows in (eng.caae_cdf(which) + (np.arange(ROWS),), eng.caae_cdf(which, sub) + (sub,)):
            assert got.shape == (len(rows), I)
            assert (np.diff(got, axis=1) >= 0).all() and (got[:, 0] > 0).all()      # non-decreasing EXACTLY
            rel = np.abs(got - want[rows]) / want[rows]
            worst = max(worst, rel.max() / tol)
            assert rel.max() <= tol, (which, rel.max(), tol)
            assert np.abs(got[:, -1] - 1.0).max() <= tol
            assert np.abs(lse - lse64[rows]).max() <= tol * np.abs(lse64).max()
        for u in (0, 6, 64):      # the resident rows are the downloaded ones
            assert eng.caae_draws("cdf_g" if which == 0 else "cdf_gpr", u).tobytes() == eng.caae_cdf(which)[0][u].tobytes()
    eng.close()
    print("CDF rows I=%d: worst relative error %.3f of the bound" % (I, worst))


# ---- draws (a), (b), (c), (e) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [64, 70, 400])
def test_draws_equal_the_restatement(I):
    urm = H.make_case(I)
    nnz = urm.nnz
    iu = np.repeat(np.arange(ROWS), np.diff(urm.indptr))
    w = _weights(urm, 4, 1, 5, scale=3.0)
    for seed in (0, 7):
        eng = _engine(urm, g_units=5, seed=seed)
        _set_state(eng, w, 1)
        n_s = eng._caae[2]
        seen = {}
        for epoch in (0, 1, 1000, 1):
            p = eng.caae_draw_perm(epoch)
            assert p.tobytes() == HC.perm(seed, epoch, nnz).tobytes(), (seed, epoch)
            assert np.array_equal(np.sort(p), np.arange(nnz))
            got = [p]
            for which in (0, 1):
                cdf = eng.caae_cdf(which)[0]      # refreshes the resident array and downloads it
                for pass_ in (0, 1):
                    neg = eng.caae_draw_negatives(epoch, pass_, which)
                    assert neg.tobytes() == HC.negatives(seed, epoch, pass_, which, cdf, iu[p]).tobytes(), (seed, epoch, which, pass_)
                    got.append(neg)
                for step in (0, 1):
                    us, nu, items, cdfb = eng.caae_draw_batch(epoch, which, step)
                    assert us.tobytes() == HC.users(seed, epoch, which, step, 32, ROWS).tobytes(), (seed, epoch, which, step)
                    if which == 0:
                        assert len(set(us.tolist())) == 32
                    assert items.tobytes() == HC.policy_items(seed, epoch, which, step, cdfb, n_s).tobytes()
                    assert items.min() >= 0 and items.max() < I
                    got += [us, items] + ([nu] if which == 0 else [])
            blob = tuple(a.tobytes() for a in got)
            if epoch in seen:
                assert seen[epoch] == blob      # the same arguments twice: the same bytes
            seen[epoch] = blob
        assert len(set(seen.values())) == 3      # different epochs: different bytes
        for q in range(len(got)):                 # ... in every kind of draw
            assert len({v[q] for v in seen.values()}) == 3, q
        assert got[1].tobytes() != got[2].tobytes() and got[3].tobytes() != got[6].tobytes() and got[4].tobytes() != got[7].tobytes()      # passes, steps
        eng.close()


# ---- weighted subset (d) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,S", [(64, 0.1), (70, 0.5), (400, 0.9)])
def test_nu_rows_have_their_size_and_no_interaction(I, S):
    from ganmf_amd.CAAE import nu_size
    from ganmf_amd.CFGAN import unpack_mask_rows
    urm = H.make_case(I)
    dense = urm.toarray() != 0
    n_free = I - dense.sum(axis=1)
    assert 0 in n_free and I in n_free
    w = _weights(urm, 4, 1, 5, scale=3.0)
    eng = _engine(urm, g_units=5, m_batch=ROWS, S=S, seed=2)
    _set_state(eng, w, 1)
    planes = {}
    for step in (0, 1, 0):
        us, nu, _, _ = eng.caae_draw_batch(3, 0, step)
        assert sorted(us.tolist()) == list(range(ROWS))
        bits = unpack_mask_rows(nu, I)
        assert not (bits & dense[us]).any()
        assert np.array_equal(bits.sum(axis=1), np.array([nu_size(int(n_free[u]), S) for u in us]))
        if step in planes:
            assert planes[step] == nu.tobytes()
        planes[step] = nu.tobytes()
    assert planes[0] != planes[1]
    eng.close()


def test_nu_statistics_against_numpy_choice():
    """Over 2000 draws at I = 100 with G' set so that r alternates between sigmoid(-6) and sigmoid(6): every item's inclusion
    frequency within 5 sigma of numpy's own choice(p=, replace=False) frequency over 2000 draws, sigma^2 = 2 p (1 - p) / 2000 with p the
    mean of the two.  Two numpy runs differ by at most 2.8 sigma at these shapes, a uniform sampler is off by 10-33 sigma."""
    from ganmf_amd.CFGAN import unpack_mask_rows
    I, E = 100, 2000
    nk = [(69, 20), (64, 32), (99, 89), (100, 30)]
    rng = np.random.RandomState(5)
    dense = np.zeros((len(nk), I), dtype=np.float32)
    for r, (n, _) in enumerate(nk):
        dense[r, rng.choice(I, size=I - n, replace=False)] = 1.0
    urm = sps.csr_matrix(dense)
    eng = _engine(urm, g_units=3, m_batch=len(nk), n_s=2, seed=3, k_rows=[k for _, k in nk])
    from ganmf_amd.CAAE import init_weights
    w = init_weights(0, len(nk), I, 4, 1, 3)
    z = np.where(np.arange(I) % 2 == 0, -6.0, 6.0).astype(np.float32)
    w["G_prime"] = [np.zeros_like(a) for a in w["G_prime"][:-1]] + [z]
    _set_state(eng, w, 1)
    weight = np.exp(1.0 / (1.0 + np.exp(-z.astype(np.float64))))
    counts = np.zeros((len(nk), I))
    for epoch in range(E):
        us, nu, _, _ = eng.caae_draw_batch(epoch, 0, 0)
        counts[us] += unpack_mask_rows(nu, I)
    eng.close()
    rs = np.random.RandomState(17)
    worst = 0.0
    for r, (n, k) in enumerate(nk):
        free = np.flatnonzero(dense[r] == 0)
        assert not counts[r, dense[r] != 0].any() and counts[r].sum() == E * k
        p = weight[free] / weight[free].sum()
        ref = np.zeros(I)
        for _ in range(E):
            ref[rs.choice(free, size=k, p=p, replace=False)] += 1
        f_dev, f_np = counts[r, free] / E, ref[free] / E
        pm = 0.5 * (f_dev + f_np)
        sigma = np.sqrt(2.0 * pm * (1.0 - pm) / E)
        z_ = np.abs(f_dev - f_np)[sigma > 0] / sigma[sigma > 0]
        assert np.all(f_dev[sigma == 0] == f_np[sigma == 0])
        worst = max(worst, z_.max())
        assert z_.max() <= 5.0, (r, z_.max())
    print("Nu statistics: worst inclusion frequency %.2f sigma from numpy's" % worst)


# Nu's keys go through the device's fast log and exp, so no host restatement is exact: its bytes are pinned by a recording instead
NU_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caae_nu_planes.npz")
NU_CASES = [(64, 0.1), (70, 0.5), (400, 0.9)]
NU_DRAWS = [(3, 0), (3, 1), (1000, 0)]


def _nu_engine(I, S, bias):
    """m_batch = 65, seed 2; every kernel and every hidden bias of G' zero, its output bias `bias`: r'_j = sigmoid(bias_j) exactly, in
    whatever order a product sums, so the planes do not depend on the GEMM planner"""
    from ganmf_amd.CAAE import init_weights
    eng = _engine(H.make_case(I), g_units=3, m_batch=ROWS, S=S, seed=2)
    w = init_weights(0, ROWS, I, 4, 1, 3)
    w["G_prime"] = [np.zeros_like(a) for a in w["G_prime"][:-1]] + [np.asarray(bias, dtype=np.float32)]
    _set_state(eng, w, 1)
    return eng


def record_nu_planes(path=NU_GOLDEN):
    """Run by hand on the device, never by the suite:
    python -c "from tests.test_gpu_caae import record_nu_planes; record_nu_planes()" """
    out = {"I": np.array([I for I, _ in NU_CASES]), "S": np.array([S for _, S in NU_CASES]), "draws": np.array(NU_DRAWS)}
    for I, S in NU_CASES:
        out["bias_%d" % I] = np.linspace(-6, 6, I).astype(np.float32)[np.random.RandomState(0).permutation(I)]
        eng = _nu_engine(I, S, out["bias_%d" % I])
        for epoch, step in NU_DRAWS:
            out["users_%d_%d_%d" % (I, epoch, step)], out["nu_%d_%d_%d" % (I, epoch, step)], _, _ = eng.caae_draw_batch(epoch, 0, step)
        eng.close()
    np.savez_compressed(path, **out)


def test_nu_planes_equal_the_recorded_bytes():
    with np.load(NU_GOLDEN) as f:
        rec = {k: f[k] for k in f.files}
    assert list(zip(rec["I"].tolist(), rec["S"].tolist())) == NU_CASES and [tuple(d) for d in rec["draws"].tolist()] == NU_DRAWS
    for I, S in NU_CASES:
        assert len(set(rec["bias_%d" % I].tolist())) == I      # not constant: every column its own weight
        eng = _nu_engine(I, S, rec["bias_%d" % I])
        for epoch, step in NU_DRAWS:
            us, nu, _, _ = eng.caae_draw_batch(epoch, 0, step)
            assert us.tobytes() == rec["users_%d_%d_%d" % (I, epoch, step)].tobytes(), (I, S, epoch, step)
            assert nu.tobytes() == rec["nu_%d_%d_%d" % (I, epoch, step)].tobytes(), (I, S, epoch, step)
        eng.close()


# ---- one D-step ----------------------------------------------------------------------------------------------------------------------
def _triples(cnt, I, rng):
    u, i, j = rng.randint(0, ROWS, cnt), rng.randint(0, I, cnt), rng.randint(0, I, cnt)
    if cnt == 64:
        u[:] = 5                      # one user fills the whole slice
    if cnt >= 3:
        i[0], j[1] = 3, 3             # one item positive and negative in the slice
        j[2] = i[2]                   # i == j
        u[cnt - 1] = u[0]             # a duplicate user, duplicate items
        i[cnt - 1] = i[0]
    return u, i, j


@pytest.mark.parametrize("k", [1, 43, 64, 65, 250])
def test_one_d_step_per_row_against_float64(k):
    I = 70
    urm = H.make_case(I)
    w = _weights(urm, k, 1, 4, scale=2.0)
    beta = 0.01
    eng = _engine(urm, k=k, d_bsize=600, beta=beta, lr=1.0)
    rng = np.random.RandomState(k)
    worst = 0.0
    for cnt in (64, 1, 130, 600):      # 600: a reference list longer than one round of the update kernel's walk (512)
        u, i, j = _triples(cnt, I, rng)
        _set_state(eng, w, 1)
        before = _get(eng, "D", 1, w)
        gens = [_get(eng, key, 1, w) for key in ("G", "G_prime")]
        loss = float(eng.caae_d_step(u, i, j))
        after = _get(eng, "D", 1, w)
        for key, old in zip(("G", "G_prime"), gens):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(old, _get(eng, key, 1, w)))
        r64, r32 = HC.CAAERef(w, beta=beta, lr=1.0), HC.CAAERef(w, beta=beta, lr=1.0, dtype=np.float32)
        (l64, g64), (l32, g32), bounds = r64.d_grads(u, i, j), r32.d_grads(u, i, j), HC.abs_d_bounds(r64, u, i, j)
        dev32 = abs(float(l32) - l64)
        assert abs(loss - l64) <= max(4.0 * dev32, 1e-5 * abs(l64)), (cnt, loss, l64, dev32)
        touched = [np.isin(np.arange(ROWS), u), np.isin(np.arange(I), np.concatenate([i, j]))]
        touched.append(touched[1])
        for n, (b0, b1, ref, ref32, bound, hit) in enumerate(zip(before, after, g64, g32, bounds, touched)):
            assert b0[~hit].tobytes() == b1[~hit].tobytes(), (cnt, n, "an untouched row changed")
            got = b0.astype(np.float64) - b1.astype(np.float64)
            ratio, bad = _ratio(got, ref, bound, b0)
            base, _ = _ratio(ref32, ref, bound, np.zeros_like(b0))
            worst = max(worst, ratio)
            assert bad.size == 0, (cnt, n, "rows with bound 0 differ", bad[:8])
            assert ratio <= allowed(base), (cnt, n, ratio, base)
    eng.close()
    print("D-step k=%d, largest row ratio: %.3g" % (k, worst))


# ---- one G-step and one G'-step ------------------------------------------------------------------------------------------------------
G_CASES = [(70, 1, 4, 32, 2, 0.1, 0.0), (400, 3, 20, 65, 40, 0.9, 0.1), (70, 1, 20, 65, 2, 0.9, 0.0), (400, 3, 4, 32, 40, 0.1, 0.1)]


def _batch(which, urm, m, n_s, rng):
    I = urm.shape[1]
    # in front the rows with 0, 1, 63, 64, 65, I - 1 and I items (those that fit)
    us = np.concatenate([np.arange(7), 7 + rng.choice(ROWS - 7, size=m - 7, replace=False)]) if m < ROWS else rng.permutation(ROWS)
    if which == 1:
        us[m - 1] = us[0]             # a G' batch repeats one user
    items = rng.randint(0, I, size=(m, n_s))
    items[1, :] = items[1, 0]         # a row whose draws repeat one item
    free = urm.toarray()[us] == 0
    nu = (rng.rand(m, I) < 0.3) & free
    return us.astype(np.int32), nu, items.astype(np.int32)


@pytest.mark.parametrize("I,gl,gu,m,n_s,lmbda,beta", G_CASES)
def test_one_g_step_per_row_against_float64(I, gl, gu, m, n_s, lmbda, beta):
    from ganmf_amd.CFGAN import pack_mask_rows
    urm = H.make_case(I)
    X = urm.toarray()
    w = _weights(urm, 6, gl, gu, scale=2.0)
    eng = _engine(urm, k=6, g_units=gu, g_layers=gl, m_batch=m, n_s=n_s, lmbda=lmbda, beta=beta, lr=1.0)
    rng = np.random.RandomState(I + gl)
    worst = 0.0
    for which, key in ((0, "G"), (1, "G_prime")):
        us, nu, items = _batch(which, urm, m, n_s, rng)
        _set_state(eng, w, gl)
        before = _get(eng, key, gl, w)
        others = [(o, _get(eng, o, gl, w)) for o in ("D", "G", "G_prime") if o != key]
        loss = float(eng.caae_g_step(which, us, pack_mask_rows(nu), items))
        after = _get(eng, key, gl, w)
        for o, old in others:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(old, _get(eng, o, gl, w))), (key, o)
        kw = dict(lmbda=lmbda, beta=beta, lr=1.0)
        r64, r32 = HC.CAAERef(w, **kw), HC.CAAERef(w, dtype=np.float32, **kw)
        nu_arg = nu if which == 0 else None
        (l64, g64), (l32, g32) = r64.g_grads(which, us, X, nu_arg, items), r32.g_grads(which, us, X, nu_arg, items)
        bounds = HC.abs_g_bounds(r64, which, us, X, nu_arg, items)
        dev32 = abs(float(l32) - l64)
        assert abs(loss - l64) <= max(4.0 * dev32, 1e-5 * abs(l64)), (key, loss, l64, dev32)
        for n, (b0, b1, ref, ref32, bound) in enumerate(zip(before, after, g64, g32, bounds)):
            got = b0.astype(np.float64) - b1.astype(np.float64)
            ratio, bad = _ratio(got, ref, bound, b0)
            base, _ = _ratio(ref32, ref, bound, np.zeros_like(b0))
            worst = max(worst, ratio)
            assert bad.size == 0, (key, n, "rows with bound 0 differ", bad[:8])
            assert ratio <= allowed(base), (key, n, ratio, base)
    eng.close()
    print("G / G' step (I=%d, %d x %d): largest row ratio %.3g" % (I, gl, gu, worst))


# ---- epoch -----------------------------------------------------------------------------------------------------------------------------
def test_epoch_equals_its_steps_and_float64():
    from ganmf_amd.CFGAN import unpack_mask_rows
    I, k, gl, gu = 70, 8, 2, 12
    urm = H.make_case(I)
    X = urm.toarray()
    iu = np.repeat(np.arange(ROWS), np.diff(urm.indptr))
    w = _weights(urm, k, gl, gu, scale=2.0)
    kw = dict(lmbda=0.5, beta=0.01, lr=1e-2)
    engines = [_engine(urm, k=k, g_units=gu, g_layers=gl, d_bsize=64, m_batch=32, seed=11, **kw) for _ in range(3)]
    for eng in engines:
        _set_state(eng, w, gl)
    a, b, c = engines
    r64, r32 = HC.CAAERef(w, **kw), HC.CAAERef(w, dtype=np.float32, **kw)
    got_l, l64, l32 = [], [], []
    for epoch in (3, 4):
        la = np.concatenate(a.caae_epoch(epoch, 2, 2, 2))
        lc = np.concatenate(c.caae_epoch(epoch, 2, 2, 2))
        assert la.tobytes() == lc.tobytes()      # two handles, one seed: the same bytes
        p = a.caae_draws("perm")
        us, pos = iu[p], urm.indices[p]
        negs = [(a.caae_draws("neg_g", q), a.caae_draws("neg_gpr", q)) for q in range(2)]
        gb = [(a.caae_draws("users_g", s), a.caae_draws("nu", s), a.caae_draws("items_g", s)) for s in range(2)]
        pb = [(a.caae_draws("users_gpr", s), a.caae_draws("items_gpr", s)) for s in range(2)]
        lb = []
        for ng, np_ in negs:
            for s in range(0, len(p), 64):
                sl = slice(s, min(s + 64, len(p)))
                lb.append(b.caae_d_step(us[sl], pos[sl], ng[sl]))
                lb.append(b.caae_d_step(us[sl], pos[sl], np_[sl]))
        lb += [b.caae_g_step(0, u_, nu, it) for u_, nu, it in gb] + [b.caae_g_step(1, u_, None, it) for u_, it in pb]
        assert la.tobytes() == np.array(lb, dtype=np.float32).tobytes()      # the epoch is its steps on its own recorded draws
        got_l.append(la.astype(np.float64))
        gbd = [(u_, unpack_mask_rows(nu, I), it) for u_, nu, it in gb]
        for ref, store in ((r64, l64), (r32, l32)):
            store.append(np.concatenate(ref.epoch(X, us, pos, negs, gbd, pb, 64)).astype(np.float64))
    errs, base = {}, {}
    for key in ("D", "G", "G_prime"):
        ta, tb, tc = (_get(eng, key, gl, w) for eng in engines)
        for n, (x, y, z, p64, p32) in enumerate(zip(ta, tb, tc, r64.p[key], r32.p[key])):
            assert x.tobytes() == y.tobytes() == z.tobytes(), (key, n)
            scale = np.abs(p64).max()
            errs["%s%d" % (key, n)] = np.abs(x - p64).max() / scale
            base["%s%d" % (key, n)] = np.abs(p32.astype(np.float64) - p64).max() / scale
    f64 = np.concatenate(l64)
    errs["loss"] = np.abs(np.concatenate(got_l) - f64).max() / np.abs(f64).max()
    base["loss"] = np.abs(np.concatenate(l32) - f64).max() / np.abs(f64).max()
    for eng in engines:
        eng.close()
    print("CAAE epoch: " + ", ".join("%s %.2g (f32 %.2g)" % (n, errs[n], base[n]) for n in sorted(errs)))
    for n, v in errs.items():
        assert v <= max(DIS_FACTOR * base[n], DIS_FLOOR), (n, v, base[n])


# ---- class -----------------------------------------------------------------------------------------------------------------------------
FIT = dict(d_steps=1, g_steps=2, gpr_steps=1, g_layers=2, g_units=6, gpr_layers=5, gpr_units=9, num_factors=5, d_bsize=256, m_batch=16,
           lmbda=0.4, beta=0.01, lr=1e-2, S=0.3)


def _restated_scores(model, ids):
    w = {key: [model.sess.run(r) for r in model.params[key]] for key in ("D", "G", "G_prime")}
    X = model._URM_fit.toarray()[ids]
    return HC.CAAERef(w).scores(X), HC.CAAERef(w, dtype=np.float32).scores(X)


@pytest.mark.parametrize("sampler", ["device", "numpy"])
def test_fit_and_scores(sampler):
    from ganmf_amd.CAAE import CAAE
    urm = H.make_case(70)
    model = CAAE(urm, mode="item", seed=4, is_experiment=True, sampler=sampler)
    np.random.seed(21)
    assert model.fit(epochs=3, **FIT) == 4
    assert len(model.train_d_loss) == 3 and np.isfinite(model.train_d_loss + model.train_pg_loss + model.train_ng_loss).all()
    assert model.config["gpr_units"] == 9 and model.sess.run(model.params["G_prime"][0]).shape == (70, 6)      # G' is built like G
    first = [model.sess.run(r) for r in model._all_refs()]
    from ganmf_amd.CAAE import init_weights
    start = init_weights(4, 65, 70, 5, 2, 6)
    for key, lo in (("D", 0), ("G", 3), ("G_prime", 9)):      # every trained tensor moved (the biases of G' included)
        for n, a in enumerate(start[key]):
            assert first[lo + n].shape == a.shape and first[lo + n].tobytes() != a.tobytes(), (key, n)
    ids = np.array([5, 0, 64, 5, 63])      # not 0..n: the reference would score rows 0..4 here
    got = model._compute_item_score(ids)
    s64, s32 = _restated_scores(model, ids)
    assert got.shape == (5, 70) and got[0].tobytes() == got[3].tobytes()
    err = np.abs(got - s64).max() / np.abs(s64).max()
    base = np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max()
    print("CAAE fit (%s): scores %.2g (f32 %.2g)" % (sampler, err, base))
    assert err <= max(DIS_FACTOR * base, DIS_FLOOR)
    assert (got > 0).all() and (got < 1).all()      # the sigmoid is applied
    model.engine.close()


@pytest.fixture(scope="module")
def fitted():
    from ganmf_amd.CAAE import CAAE
    urm = H.make_case(70, seed=3)
    model = CAAE(urm, seed=9, is_experiment=True)
    model.fit(epochs=2, **FIT)
    rng = np.random.RandomState(31)
    t = ((rng.rand(*urm.shape) < 0.15) & (urm.toarray() == 0)) * rng.randint(1, 6, size=urm.shape)
    yield model, urm, sps.csr_matrix(t.astype(np.float32))
    model.engine.close()


@pytest.mark.parametrize("full", [False, True])
def test_device_evaluation_equals_the_host_evaluator(fitted, full):
    from ganmf_amd.base import BaseRecommender
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    model, urm, test = fitted

    class Twin(BaseRecommender):
        def _compute_item_score(self, user_id_array, items_to_compute=None):
            return model._compute_item_score(user_id_array).astype(np.float64)
    cut = [1, 5, 10]
    ev = EvaluatorHoldoutFast(test, cut, full_metrics=full)
    assert ev.use_device_metrics
    dev, _ = ev.evaluateRecommender(model)
    host, _ = EvaluatorHoldoutFast(test, cut, full_metrics=full).evaluateRecommender(Twin(urm))
    for c in cut:
        assert set(dev[c]) == set(host[c])
        for name, v in host[c].items():
            if name == "RMSE" and not full:
                assert np.isnan(dev[c][name]) and np.isnan(v)
                continue
            assert abs(dev[c][name] - v) <= (1e-5 if name == "RMSE" else 1e-12) * max(1.0, abs(v)), (c, name, dev[c][name], v)
    items = model.recommend(np.arange(8), cutoff=5)
    seen = urm.toarray() != 0
    assert all(not seen[u, i] for u in range(8) for i in items[u])


def test_early_stopping_restores_every_tensor():
    from ganmf_amd.CAAE import CAAE

    class Watch(object):
        def __init__(self):
            self.values, self.states = [0.5, 0.4, 0.3, 0.9], []

        def evaluateRecommender(self, m):
            self.states.append([m.sess.run(r) for r in m._all_refs()])
            return {5: {"MAP": self.values[len(self.states) - 1]}}, ""
    urm = H.make_case(70, seed=3)
    model = CAAE(urm, seed=9, is_experiment=True)
    watch = Watch()
    assert model.fit(epochs=10, allow_worse=1, freq=1, validation_evaluator=watch, **FIT) == 3
    assert len(watch.states) == 3
    now = [model.sess.run(r) for r in model._all_refs()]
    assert len(now) == 3 + 6 + 6
    for a, best, last in zip(now, watch.states[0], watch.states[2]):
        assert a.tobytes() == best.tobytes() and a.tobytes() != last.tobytes()
    model.engine.close()


def test_bundle_names_and_round_trip(fitted, tmp_path):
    from ganmf_amd.CAAE import CAAE
    from ganmf_amd.tf_bundle import read_bundle
    model, urm, _ = fitted
    model.saveModel(str(tmp_path), "caae_ckpt")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["caae_ckpt.data-00000-of-00001", "caae_ckpt.index"]
    data = read_bundle(str(tmp_path / "caae_ckpt"))
    want = {"D/disc_user_embeddings": (65, 5), "D/disc_item_embeddings": (70, 5), "D/disc_item_bias": (70,)}
    for scope, stem in (("G", "g"), ("G_prime", "gpr")):
        for l in range(2):
            want["%s/%s_layer_%d/kernel" % (scope, stem, l)] = (70 if l == 0 else 6, 6)
            want["%s/%s_layer_%d/bias" % (scope, stem, l)] = (6,)
        want["%s/%s_reconstruction/kernel" % (scope, stem)] = (6, 70)
        want["%s/%s_reconstruction/bias" % (scope, stem)] = (70,)
    assert {k_: v.shape for k_, v in data.items()} == want
    assert [r.name for r in model._all_refs()] == (
        ["D/disc_user_embeddings", "D/disc_item_embeddings", "D/disc_item_bias"]
        + ["G/g_layer_0/kernel", "G/g_layer_0/bias", "G/g_layer_1/kernel", "G/g_layer_1/bias", "G/g_reconstruction/kernel",
           "G/g_reconstruction/bias"]
        + ["G_prime/gpr_layer_0/kernel", "G_prime/gpr_layer_0/bias", "G_prime/gpr_layer_1/kernel", "G_prime/gpr_layer_1/bias",
           "G_prime/gpr_reconstruction/kernel", "G_prime/gpr_reconstruction/bias"])
    twin = CAAE(urm, is_experiment=True)
    twin.load_bundle(str(tmp_path), "caae_ckpt")
    ids = np.arange(urm.shape[0])
    assert twin._compute_item_score(ids).tobytes() == model._compute_item_score(ids).tobytes()
    for a, b in zip(twin._all_refs(), model._all_refs()):
        assert twin.sess.run(a).tobytes() == model.sess.run(b).tobytes()
    twin.engine.close()


def test_wrong_model_entries_refuse():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = H.make_case(70)
    eng = _engine(urm)
    ids = np.arange(4, dtype=np.int32)
    calls = [lambda: eng.train_epoch(np.arange(ROWS)), lambda: eng.train_step(0, ids), lambda: eng.discriminate(ids),
             lambda: eng.als_half_sweep(0, 0.1), lambda: eng.pure_svd(np.zeros((65, 4), np.float32), 1),
             lambda: eng.itemknn_fit(L.ITEMKNN_PRODUCT, 5), lambda: eng.slim_bpr_init(), lambda: eng.comm_init_local(1),
             lambda: eng.recommend_candidates(ids, 3), lambda: eng.bench_scores(4)]
    for call in calls:      # other models' entries: the message names this one
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_CAAE"):
            call()
    for call in (lambda: eng.cfgan_draw_masks(0), lambda: eng.cfgan_step(0, 0, 4), lambda: eng.cfgan_masks(),
                 lambda: eng.cfgan_init(4, 1, "linear", 32, 32, "ZR", 0.0, 0, np.zeros(ROWS)), lambda: eng.cfgan_epoch(0)):
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_CFGAN"):
            call()
    for call in (lambda: eng.caae_init(4, 1, 64, 32, 4, 0.5, 0.0, 0.1, 0, np.zeros(ROWS)),      # initialised already
                 lambda: eng.caae_d_step([0], [70], [0]), lambda: eng.caae_d_step(np.zeros(65), np.zeros(65), np.zeros(65)),
                 lambda: eng.caae_cdf(2), lambda: eng.scores(ids, transposed=True), lambda: eng.get_tensor(L.T_CAAE_G0 + 4),
                 lambda: eng.caae_draws("neg_g", 0)):
        with pytest.raises(L.GanmfError):
            call()
    assert eng.get_tensor(L.T_CAAE_GPR0 + 3).shape == (1, 70) and eng.get_tensor(L.T_USER_EMB).shape == (65, 4)
    eng.close()
    cf = Engine(ROWS, 70, 1, 4, 32, model=L.MODEL_CFGAN, d_layers=1, d_act="linear")
    cf.set_urm(urm)
    cf.cfgan_init(4, 1, "linear", 32, 32, "ZR", 0.0, 0, np.zeros(ROWS))
    cf._caae = (64, 32, 4)
    caae_calls = [lambda: cf.caae_init(4, 1, 64, 32, 4, 0.5, 0.0, 0.1, 0, np.zeros(ROWS)), lambda: cf.caae_cdf(0),
                  lambda: cf.caae_draw_perm(0), lambda: cf.caae_draw_negatives(0, 0, 0), lambda: cf.caae_draw_batch(0, 0, 0),
                  lambda: cf.caae_draws("perm"), lambda: cf.caae_d_step([0], [0], [0]),
                  lambda: cf.caae_g_step(1, np.zeros(32), None, np.zeros((32, 4))), lambda: cf.caae_epoch(0)]
    for call in caae_calls:      # every ganmf_caae_* entry refuses a CFGAN handle
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_CAAE"):
            call()
    cf.close()
    with pytest.raises(L.GanmfError, match="single-GPU"):
        Engine(ROWS, 70, 4, 1, 1, model=L.MODEL_CAAE, world_size=2)
    with pytest.raises(L.GanmfError, match="fp32-accurate"):
        Engine(ROWS, 70, 4, 1, 1, model=L.MODEL_CAAE, mfma="bf16")
    with pytest.raises(L.GanmfError, match="256"):
        Engine(ROWS, 70, 257, 1, 1, model=L.MODEL_CAAE)
