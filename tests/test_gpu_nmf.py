"""NMF on the device: ganmf_nmf_mu / ganmf_nmf_cd / ganmf_nmf_error against the numpy restatement (tests/helpers_nmf.py) at fixed
iteration counts, the nndsvda start from the device's own SVD, pad columns, signs, determinism and errors, and NMFRecommender end
to end against the golden fixture (tests/golden/nmf_tiny.npz: sklearn's own results, so no test here needs sklearn).

Tolerances are MEASURED, not fixed (as in tests/test_gpu_puresvd.py).  Per case the float64 restatement, the float32 restatement and
the device start from the same W, H and permutations and stop after 1, 10 and 50 iterations; at every stop
    e_prod = max |W H - W64 H64| / max |W64 H64|,   e_err = |error - error64| / error64
and each figure of the device must be <= 4 x the float32 restatement's figure of the same kind at the same stop (4 as in
test_gpu_ials.py: another summation order is backward stable with the same scaling).  The restatement's e_err is one float32 number's
distance from float64 and can fall far below one rounding by chance, so that yardstick has a floor of eps32 = 2^-23: the bound on the
device's e_err is 4 x max(e_err of the restatement, eps32), as in test_error_entry_against_the_restatement_on_the_start.  The
device's error scalar is ganmf_nmf_error's, the restatement's is helpers_nmf.divergence in the restatement's own type.  Coordinate
descent also returns its violation, a sum of |projected gradients| that goes to zero, so only its absolute error means something: the
host divides it by the first iteration's violation and compares with tol = 1e-4, and |violation - violation64| / first violation64
must stay below tol / 100 (float32 rounding of the gradients leaves 1e-8 .. 1e-7 there; a wrong projection rule or a missed row is
of order 1).  All figures are printed.  For coordinate descent the comparison presupposes that the two restatements end every stop
with the same zero pattern (a coordinate that float32 clips at max(., 0) and float64 does not is a different active set, not
rounding): that is asserted first, as a precondition; the seeds are ones for which it holds.

Pad columns.  get_tensor returns the k real columns only, so after EVERY entry the factors read back are uploaded into a second
handle -- whose pad columns are zero by construction -- and everything that reads a factor row over its padded width must return
the same bytes from both handles: the scoring product (every pad column) and the Kullback-Leibler error (the sampled product reads
whole float4 groups).

The shapes are the smallest that reach each branch: k = 1; k on both sides of 16, 32 and 64 (the sampled product gives an entry 4, 8
or 16 lanes as k passes 16 and 32, a lane group of the sparse product covers four columns, a wave of the coordinate-descent kernel
64: k = 32, 33, 64, 65 change the layout); both orientations; k = MAX_FACTORS (five registers per lane); every matrix has a row
and a column without an entry and a row of 40 entries, longer than the 16 a row's lane groups of the sparse product take per
round; 300 x 200 stores 9 000 entries, more than one 256-entry chunk per workgroup of the sampled product."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_nmf as HN

pytestmark = pytest.mark.gpu

FACTOR = 4.0
TOL = 1e-4      # sklearn's tol, what violation / first violation is compared with
ITERS = (1, 10, 50)
MAX_FACTORS = 270
# (n_users, n_items, k, stops, seed)
CASES = [(40, 30, 1, ITERS, 1), (40, 30, 4, ITERS, 1), (130, 70, 9, ITERS, 1), (70, 130, 9, ITERS, 1), (300, 200, 32, ITERS, 2),
         (300, 200, 33, ITERS, 1), (300, 200, 64, ITERS, 1), (300, 200, 65, ITERS, 5), (300, 290, MAX_FACTORS, (5,), 1)]
SOLVERS = {"mu_fro": HN.FROBENIUS, "mu_kl": HN.KULLBACK_LEIBLER, "cd": HN.FROBENIUS}


def _inputs(case):
    n_users, n_items, k, stops, seed = CASES[case]
    X = HN.case_matrix(n_users, n_items, seed)
    W0, H0 = HN.start_factors(X, k, seed + 100)
    rng = np.random.RandomState(seed + 200)
    perms = np.array([[rng.permutation(k), rng.permutation(k)] for _ in range(max(stops))])
    return X, W0, H0, perms


def _start(X, W0, k, tag, update_H):
    """the fit's start, or sklearn's start of transform: sqrt(mean / k) everywhere for the multiplicative update, zeros for cd"""
    if update_H:
        return W0
    return np.zeros_like(W0) if tag == "cd" else np.full_like(W0, np.sqrt(X.mean() / k))


@functools.lru_cache(maxsize=None)
def _reference(case, tag, update_H, dtype_name):
    """[(W, H, error, violation of the last iteration or None, violation of the first or None)] at every stop, in the restatement's
    own type; computed once"""
    dtype = np.dtype(dtype_name).type
    X, W0, H0, perms = _inputs(case)
    k, stops = CASES[case][2], CASES[case][3]
    W, H = _start(X, W0, k, tag, update_H), H0
    out, done, first = [], 0, None
    for n in stops:
        viol = None
        if tag == "cd":
            pm = perms[done:n] if update_H else perms[done:n, :1]
            W, H, v = HN.cd(X, W, H, pm, update_H, dtype)
            viol = float(v[-1])
            first = float(v[0]) if first is None else first
        else:
            W, H = HN.mu(X, W, H, SOLVERS[tag], n - done, update_H, dtype)
        done = n
        out.append((W, H, HN.divergence(X, W, H, SOLVERS[tag], dtype), viol, first))
    return out


def _engine(X, k):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(X.shape[0], X.shape[1], k, 1, 1, model=L.MODEL_MF)
    eng.set_confidence(0, X)
    eng.set_confidence(1, sps.csr_matrix(X.T))
    return eng


def _set(eng, W, H):
    from ganmf_amd import _lib as L
    eng.set_tensor(L.T_USER_EMB, W)
    eng.set_tensor(L.T_ITEM_EMB, np.ascontiguousarray(np.asarray(H).T))


def _factors(eng):
    from ganmf_amd import _lib as L
    return eng.get_tensor(L.T_USER_EMB), np.ascontiguousarray(eng.get_tensor(L.T_ITEM_EMB).T)


def _advance(eng, tag, n, perms, update_H):
    """n more iterations on the device: (error, violation of the last iteration or None)"""
    if tag == "cd":
        viol = eng.nmf_cd(perms if update_H else perms[:, :1], update_H)
        assert viol.shape == (n,) and np.isfinite(viol).all() and (viol >= 0).all()
        return eng.nmf_error(HN.FROBENIUS), float(viol[-1])
    return eng.nmf_mu(SOLVERS[tag], n, update_H, error=True), None


@pytest.mark.parametrize("update_H", [True, False], ids=["fit", "transform"])
@pytest.mark.parametrize("tag", sorted(SOLVERS))
@pytest.mark.parametrize("case", range(len(CASES)), ids=["%dx%d-k%d" % c[:3] for c in CASES])
def test_fixed_iteration_parity(case, tag, update_H):
    n_users, n_items, k, stops, _ = CASES[case]
    X, W0, H0, perms = _inputs(case)
    ref64, ref32 = _reference(case, tag, update_H, "float64"), _reference(case, tag, update_H, "float32")
    if tag == "cd":      # precondition of the comparison, not a property of the code
        for (W64, H64, _, _, _), (W32, H32, _, _, _) in zip(ref64, ref32):
            assert np.array_equal(W64 == 0, W32 == 0) and np.array_equal(H64 == 0, H32 == 0), "pick another seed"
    eng, clean = _engine(X, k), _engine(X, k)
    try:
        _set(eng, _start(X, W0, k, tag, update_H), H0)
        done = 0
        for stop, n in enumerate(stops):
            err, viol = _advance(eng, tag, n - done, perms[done:n], update_H)
            done = n
            W, H = _factors(eng)
            W64, H64, err64, viol64, first64 = ref64[stop]
            W32, H32, err32, viol32, _ = ref32[stop]
            d_prod, y_prod = HN.product_error(W, H, W64, H64), HN.product_error(W32, H32, W64, H64)
            d_err, y_err = HN.scalar_error(err, err64), HN.scalar_error(err32, err64)
            line = "nmf parity %dx%d k=%d %s %s n=%d: e_prod device %.3e float32 %.3e ratio %.2f | error %.6f e_err device %.3e float32 %.3e" % (
                n_users, n_items, k, tag, "fit" if update_H else "transform", n, d_prod, y_prod, d_prod / y_prod, err, d_err, y_err)
            if tag == "cd":
                d_viol, y_viol = abs(viol - viol64) / first64, abs(viol32 - viol64) / first64
                line += " | violation %.6g of %.6g e_viol device %.3e float32 %.3e" % (viol, first64, d_viol, y_viol)
            print(line)
            assert np.isfinite(W).all() and np.isfinite(H).all() and (W >= 0).all() and (H >= 0).all() and np.isfinite(err)
            assert d_prod <= FACTOR * y_prod, (n, d_prod, y_prod)
            assert d_err <= FACTOR * max(y_err, HN.EPS), (n, d_err, y_err)
            if tag == "cd":
                assert d_viol <= TOL / 100, (n, d_viol, y_viol)
            if not update_H:
                assert np.array_equal(H, H0)      # transform leaves H alone, bit for bit
            # pad columns are zero after this entry: the same bytes as from a handle whose pads are zero by construction
            _set(clean, W, H)
            s = eng.scores(np.arange(n_users))
            assert s.tobytes() == clean.scores(np.arange(n_users)).tobytes()
            assert eng.nmf_error(HN.KULLBACK_LEIBLER) == clean.nmf_error(HN.KULLBACK_LEIBLER)
            assert eng.nmf_error(HN.FROBENIUS) == clean.nmf_error(HN.FROBENIUS)
        want = W.astype(np.float64).dot(H.astype(np.float64))
        assert np.abs(s - want).max() <= 1e-5 * np.abs(want).max()
        # the multiplicative update keeps a row / a column without an entry at exact zeros under the Frobenius loss
        if tag == "mu_fro":
            assert not W[0].any() and (not update_H or not H[:, 1].any())
    finally:
        eng.close()
        clean.close()


@pytest.mark.parametrize("case", [2, 7, 8], ids=["%dx%d-k%d" % CASES[c][:3] for c in (2, 7, 8)])
@pytest.mark.parametrize("tag", sorted(SOLVERS))
def test_two_runs_return_the_same_bytes(tag, case):
    X, W0, H0, perms = _inputs(case)
    n = min(10, max(CASES[case][3]))
    got = []
    for _ in range(2):
        eng = _engine(X, CASES[case][2])
        try:
            _set(eng, W0, H0)
            err, viol = _advance(eng, tag, n, perms[:n], True)
            W, H = _factors(eng)
            again = eng.nmf_error(SOLVERS[tag])
            got.append((W.tobytes(), H.tobytes(), err, viol, again))
        finally:
            eng.close()
    assert got[0] == got[1] and got[0][2] == got[0][4]      # and the error entry repeats what the solver's call returned


def test_error_entry_against_the_restatement_on_the_start():
    """ganmf_nmf_error alone, both losses, on factors no solver has touched: float64 accumulation of float32 products"""
    X, W0, H0, _ = _inputs(2)
    eng = _engine(X, 9)
    try:
        _set(eng, W0, H0)
        for beta in (HN.FROBENIUS, HN.KULLBACK_LEIBLER):
            got, want, f32 = eng.nmf_error(beta), HN.divergence(X, W0, H0, beta), HN.divergence(X, W0, H0, beta, np.float32)
            print("nmf error entry beta=%d: device %.9g float64 %.9g float32 %.9g" % (beta, got, want, f32))
            assert HN.scalar_error(got, want) <= FACTOR * max(HN.scalar_error(f32, want), HN.EPS)
        W, H = _factors(eng)
        assert W.tobytes() == W0.tobytes() and H.tobytes() == H0.tobytes()
    finally:
        eng.close()


def test_argument_errors_leave_the_factors_unchanged():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    X, W0, H0, perms = _inputs(1)
    eng = Engine(40, 30, 4, 1, 1, model=L.MODEL_MF)
    try:
        _set(eng, W0, H0)
        calls = [lambda: eng.nmf_mu(0, 1), lambda: eng.nmf_cd(perms[:1]), lambda: eng.nmf_error(0)]
        for call in calls:      # no side uploaded, then only side 0
            with pytest.raises(L.GanmfError, match="ganmf_als_set_confidence has not been called for both sides") as err:
                call()
            assert "(-1)" in str(err.value)
        eng.set_confidence(0, X)
        for call in calls:
            with pytest.raises(L.GanmfError, match="has not been called for both sides"):
                call()
        eng.set_confidence(1, sps.csr_matrix(X.T))
        with pytest.raises(L.GanmfError, match=r"\(-1\).*beta_loss must be"):
            eng.nmf_mu(2, 1)
        with pytest.raises(L.GanmfError, match=r"\(-1\).*beta_loss must be"):
            eng.nmf_error(-1)
        with pytest.raises(L.GanmfError, match=r"\(-1\).*n_iter -1 is negative"):
            eng.nmf_mu(0, -1)
        bad = perms[:2].copy()
        bad[1, 1, 2] = bad[1, 1, 3]
        with pytest.raises(L.GanmfError, match=r"\(-1\).*permutation 3 is not a permutation of 0 \.\. 3"):
            eng.nmf_cd(bad)
        bad[1, 1, 2] = 4
        with pytest.raises(L.GanmfError, match=r"\(-1\).*permutation 3 is not a permutation"):
            eng.nmf_cd(bad)
        W, H = _factors(eng)
        assert W.tobytes() == W0.tobytes() and H.tobytes() == H0.tobytes()
        assert eng.nmf_cd(perms[:0]).shape == (0,)      # no iteration: nothing runs
        assert _factors(eng)[0].tobytes() == W0.tobytes()
    finally:
        eng.close()
    wide = Engine(300, 290, MAX_FACTORS + 1, 1, 1, model=L.MODEL_MF)
    try:
        m = sps.identity(300, dtype=np.float32, format="csr")[:, :290]
        wide.set_confidence(0, sps.csr_matrix(m))
        wide.set_confidence(1, sps.csr_matrix(m.T))
        with pytest.raises(L.GanmfError, match=r"\(-1\).*above the limit of %d" % MAX_FACTORS):
            wide.nmf_mu(0, 1)
    finally:
        wide.close()
    sharded = Engine(40, 30, 4, 4, 8, world_size=2, rank=0)      # rank 0 of a two-rank loopback group (tests/test_gpu_dist_local.py)
    try:
        sharded.comm_init_local(4243)
        sharded.set_confidence(0, X)
        sharded.set_confidence(1, sps.csr_matrix(X.T))
        with pytest.raises(L.GanmfError, match="single-GPU entry"):
            sharded.nmf_mu(0, 1)
    finally:
        sharded.close()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "nmf_tiny.npz"))


def _matrix(fx, c):
    return sps.csr_matrix((fx[c + "/X_data"], fx[c + "/X_indices"], fx[c + "/X_indptr"]), shape=tuple(fx[c + "/shape"]))


@pytest.mark.parametrize("case", ["a", "b"])
def test_nndsvda_start_from_the_device_s_own_svd(fx, case):
    from ganmf_amd import _lib as L
    from ganmf_amd.NMF import NMFRecommender, nndsvda_split
    from ganmf_amd.PureSVD import svd_plan
    X, k, seed = _matrix(fx, case), int(fx[case + "/k"]), int(fx[case + "/seed"])
    model = NMFRecommender(X)
    model._build(k)
    try:
        model.engine.set_confidence(0, X)
        model.engine.set_confidence(1, sps.csr_matrix(X.T))
        np.random.seed(seed)
        W, H = model._initial_factors(X, k, "nndsvda")
        # the stream stands where sklearn's randomized_svd leaves it: one normal draw of [min(shape), k + 10]
        after = np.random.random_sample()
        n_random, n_iter, _ = svd_plan(X.shape[0], X.shape[1], k)
        np.random.seed(seed)
        np.random.normal(size=(min(X.shape), n_random))
        assert after == np.random.random_sample()
        # the split of the device's own SVD is the numpy split, exactly
        U = model.engine.get_tensor(L.T_USER_EMB)
        item = model.engine.get_tensor(L.T_ITEM_EMB)
        S = np.sqrt((item.astype(np.float64) ** 2).sum(0))
        np.random.seed(seed)
        S_dev = model.engine.pure_svd(np.random.normal(size=(min(X.shape), n_random)), n_iter)
        W2, H2 = nndsvda_split(model.engine.get_tensor(L.T_USER_EMB), S_dev,
                               np.ascontiguousarray((model.engine.get_tensor(L.T_ITEM_EMB) / S_dev).T), X.mean())
        assert W.tobytes() == W2.tobytes() and H.tobytes() == H2.tobytes()
        assert np.allclose(S, S_dev, rtol=1e-5) and U.shape == (X.shape[0], k)
        assert W.dtype == np.float32 and (W > 0).all() and (H > 0).all()
        # against sklearn's start: entries within 1e-7 of the 1e-6 threshold are left out (at most 1 %); the others agree to what
        # float32 leaves of a singular vector, eps32 / (relative gap >= 5e-3, tools/make_nmf_fixture.py) = 2.4e-5, times 4, of the largest entry
        for name, got, want in (("W0", W, fx[case + "/nndsvda_W0"]), ("H0", H, fx[case + "/nndsvda_H0"])):
            near = np.abs(np.minimum(got, want).astype(np.float64) - 1e-6) <= 1e-7
            diff = np.abs(got - want)[~near].max() / want.max()
            print("nmf nndsvda %s %s: left out %d of %d, largest difference %.3e of the largest entry" % (case, name, near.sum(), near.size, diff))
            assert near.mean() <= 0.01
            assert diff <= FACTOR * HN.EPS / 5e-3
    finally:
        if model.engine is not None:
            model.engine.close()


def _counted(model, name):
    got = []
    inner = getattr(model, name)

    def wrapper(*a, **kw):
        got.append(inner(*a, **kw))
        return got[-1]
    setattr(model, name, wrapper)
    return got


E2E_ARGS = {"mu": "multiplicative_update", "cd": "coordinate_descent"}


@pytest.mark.parametrize("config", range(5))
def test_fit_end_to_end_against_sklearn_s_records(fx, config):
    """fit() at the reference's settings after np.random.seed(0): the reconstruction error is no worse than sklearn's own of the
    same seed plus the spread (max - min) of sklearn's five seeds -- a run of hundreds of iterations amplifies float32's rounding into
    another local minimum as another seed does"""
    from MatrixFactorization.NMFRecommender import NMFRecommender
    solver, loss, init = str(fx["e2e/configs"][config]).split("|")
    errs, n_iters = fx["e2e/err"][config], fx["e2e/n_iter"][config]
    X, k = _matrix(fx, "b"), int(fx["b/k"])
    model = NMFRecommender(X)
    try:
        np.random.seed(0)
        model.fit(num_factors=k, solver=E2E_ARGS[solver], init_type=init, beta_loss=loss)
        bound = errs[0] + (errs.max() - errs.min())
        print("nmf fit %s %s %s: n_iter_ %d (sklearn %d, its seeds %s) transform %d | reconstruction_err_ %.4f sklearn %.4f bound %.4f" % (
            solver, loss, init, model.n_iter_, n_iters[0], n_iters.tolist(), model.transform_n_iter_, model.reconstruction_err_, errs[0], bound))
        assert model.reconstruction_err_ <= bound
        assert 1 <= model.n_iter_ <= 500 and 1 <= model.transform_n_iter_ <= 500
        if solver == "mu":
            assert model.n_iter_ % 10 == 0
        W, Ht = model.USER_factors, model.ITEM_factors
        assert W.shape == (130, k) and Ht.shape == (70, k) and np.isfinite(W).all() and np.isfinite(Ht).all()
        assert (W >= 0).all() and (Ht >= 0).all()
        # USER_factors is transform's solve: its error with the fit's H is close to the fit's own, and reconstruction_err_ is the FIT's
        beta = SOLVERS["mu_kl"] if loss == "kullback-leibler" else HN.FROBENIUS
        assert model.engine.nmf_error(beta) == pytest.approx(HN.divergence(X, W, Ht.T, beta), rel=1e-5)
    finally:
        if model.engine is not None:
            model.engine.close()


def test_recommend_evaluate_and_persistence_on_the_fitted_model(fx, tmp_path):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from MatrixFactorization.NMFRecommender import NMFRecommender
    X, k = _matrix(fx, "b"), int(fx["b/k"])
    model = NMFRecommender(X)
    try:
        np.random.seed(0)
        model.fit(num_factors=k)
        W, Ht = model.USER_factors, model.ITEM_factors
        S = W.astype(np.float64).dot(Ht.astype(np.float64).T)
        seen = np.asarray(X.todense()) != 0
        masked = np.where(seen, -np.inf, S)
        warm = [u for u in range(130) if X[u].nnz > 0]
        lists = model.recommend(warm, cutoff=5)
        compared = 0
        for u, got in zip(warm, lists):
            order = np.argsort(-masked[u], kind="stable")
            top = masked[u][order]
            if np.min(top[:5] - top[1:6]) > 1e-5 * np.abs(S).max():      # further apart at the cut than the float32 scoring product's error
                assert list(got) == list(order[:5]), u
                compared += 1
        assert compared >= 30
        assert model.recommend(0, cutoff=5) == []                 # the user without an entry is cold under the MF contract
        rng = np.random.RandomState(4)
        test = sps.csr_matrix(((~seen) * (rng.rand(130, 70) < 0.15)) * rng.randint(1, 6, (130, 70)), dtype=np.float32)
        hook = _counted(model, "evaluate_on_device")
        results, _ = EvaluatorHoldoutFast(test, [5]).evaluateRecommender(model)
        assert len(hook) >= 1 and all(r is not None for r in hook)
        assert 0.0 < results[5]["MAP"] <= 1.0
        # saveModel -> a fresh instance's loadModel -> the same score bytes
        before = model._compute_item_score(warm)
        model.saveModel(str(tmp_path))
        fresh = NMFRecommender(X)
        fresh.loadModel(str(tmp_path))
        try:
            assert fresh._compute_item_score(warm).tobytes() == before.tobytes()
            assert fresh.USER_factors.tobytes() == W.tobytes()
        finally:
            fresh.engine.close()
    finally:
        if model.engine is not None:
            model.engine.close()
