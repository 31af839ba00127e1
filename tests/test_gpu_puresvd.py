"""PureSVD on the device: ganmf_pure_svd against the numpy restatement (tests/helpers_puresvd.py), its pad columns, sign rule,
determinism and errors, and PureSVDRecommender end to end against the golden fixture (tests/golden/puresvd_tiny.npz: sklearn's own
result, so no test here needs sklearn).

Tolerances are MEASURED, not fixed (as in tests/test_gpu_ials.py).  Per case the float64 restatement, the float32 restatement and
the device start from the same omega; with S = USER . ITEM^T,
    e_score = max |S - S64| / max |S64|,   e_sigma = max |sigma - sigma64| / sigma_1 (from the returned sigma AND from ITEM's column norms),
    e_orth  = max |O^T O - I| of the orthonormal factor O (USER, or ITEM / sigma in the transposed case).
The device's e_score and e_sigma must be <= 4 x the float32 restatement's e_score (a singular value cannot move by more than the
spectral norm of the score error; the restatement's own e_sigma sits at one or two ulps, too noisy a yardstick), its e_orth <= 4 x the
restatement's e_orth.  4 as in test_gpu_ials.py: another summation order is backward stable with the same scaling.  All figures are
printed; the first MI355X run's are in profiles/puresvd_parity.md.  Both errors scale with 1 / (sigma_k - sigma_{k+1}): every case
asserts a relative gap of at least 1e-3 by a float64 dense SVD first.

The shapes are the smallest that reach each branch: l = k + 10 on both sides of 32 and 64 (a lane group of the sparse product covers
four columns: l = 32, 33, 64, 65 change its layout), a row longer than every gather stride, both orientations, n_iter = 7 and 4 and 0,
l = 256, 260 and SVD_MAX_RANDOM.  (257 x 131 at k = 13 runs n_iter = 7 by sklearn's rule, 13 < 13.1; n_iter = 4 is reached by every
900 x 800 case.)"""
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_puresvd as H

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _engine(urm, k):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(urm.shape[0], urm.shape[1], k, 1, 1, model=L.MODEL_MF)
    eng.set_confidence(0, urm)
    eng.set_confidence(1, sps.csr_matrix(urm.T))
    return eng


def _factors(eng):
    from ganmf_amd import _lib as L
    return eng.get_tensor(L.T_USER_EMB), eng.get_tensor(L.T_ITEM_EMB)


def _check(urm, k, seed, label, n_iter=None):
    n_users, n_items = urm.shape
    n_random, auto_iter, transposed = H.plan(n_users, n_items, k)
    n_iter = auto_iter if n_iter is None else n_iter
    gap = H.relative_gap(urm, k)
    assert gap >= 1e-3, (label, gap)      # precondition of the comparison, not a property of the code
    omega = np.random.RandomState(seed).normal(size=(min(n_users, n_items), n_random))
    u64, i64, s64 = H.pure_svd(urm, omega, k, n_iter, np.float64)
    u32, i32, s32 = H.pure_svd(urm, omega, k, n_iter, np.float32)
    eng = _engine(urm, k)
    try:
        sigma = eng.pure_svd(omega, n_iter)
        user, item = _factors(eng)
        d_score, d_sigma, d_norm, d_orth = H.errors(user, item, sigma, u64, i64, s64, transposed)
        h_score, h_sigma, h_norm, h_orth = H.errors(u32, i32, s32, u64, i64, s64, transposed)
        print("puresvd parity %s n_iter=%d gap %.1e: e_score device %.3e float32 %.3e ratio %.2f | e_sigma device %.3e (norms %.3e) "
              "float32 %.3e | e_orth device %.3e float32 %.3e ratio %.2f" % (label, n_iter, gap, d_score, h_score, d_score / h_score, d_sigma,
                                                                           d_norm, h_sigma, d_orth, h_orth, d_orth / h_orth))
        assert np.isfinite(user).all() and np.isfinite(item).all() and np.isfinite(sigma).all()
        assert d_score <= FACTOR * h_score, (label, d_score, h_score)
        assert d_sigma <= FACTOR * h_score and d_norm <= FACTOR * h_score, (label, d_sigma, d_norm, h_score)
        assert d_orth <= FACTOR * h_orth, (label, d_orth, h_orth)
        # the sign rule: every column of USER has its entry of largest magnitude positive
        assert (user[np.abs(user).argmax(axis=0), np.arange(k)] > 0).all()
        # a user / an item without a stored entry has a factor row of exact zeros
        assert not user[0].any() and not item[1].any()
        # pad columns are zero: the scoring product reads the factor rows over their padded width (test_gpu_ials.py:75-79)
        s = eng.scores(np.arange(n_users))
        want = user.astype(np.float64).dot(item.astype(np.float64).T)
        bound = (np.abs(user).astype(np.float64).dot(np.abs(item).astype(np.float64).T)).max()
        assert np.abs(s - want).max() <= 1e-5 * bound
    finally:
        eng.close()


@pytest.mark.parametrize("k", [1, 3])
def test_tiny_matrix_with_empty_row_and_column(k):
    _check(H.case_matrix(40, 30, 1), k, 10 + k, "40x30 k=%d" % k)


@pytest.mark.parametrize("shape", [(400, 300), (300, 400)])
@pytest.mark.parametrize("k", [22, 23, 54, 55])
def test_width_boundaries_in_both_orientations(k, shape):
    urm = H.gap_matrix(shape[0], shape[1], k, k, long_row=200)
    assert np.diff(urm.indptr).max() >= 199
    _check(urm, k, 20 + k, "%dx%d k=%d" % (shape[0], shape[1], k))


@pytest.mark.parametrize("shape,seed", [((257, 131), 1), ((131, 257), 2)])
def test_thirteen_factors_in_both_orientations(shape, seed):
    _check(H.case_matrix(shape[0], shape[1], seed, long_row=100), 13, 30 + seed, "%dx%d k=13" % shape)


@pytest.mark.parametrize("shape", [(900, 800), (800, 900)])
@pytest.mark.parametrize("k", [246, 250, "max"])
def test_largest_ranks(k, shape):
    from ganmf_amd import _lib as L
    k = L.SVD_MAX_RANDOM - 10 if k == "max" else k
    _check(H.gap_matrix(shape[0], shape[1], k, k, long_row=200), k, 40 + k, "%dx%d k=%d" % (shape[0], shape[1], k))


def test_without_power_iteration():
    _check(H.gap_matrix(257, 131, 13, 5, long_row=100), 13, 50, "257x131 k=13", n_iter=0)


@pytest.mark.parametrize("k", [13, 55])
def test_two_calls_return_the_same_bytes(k):
    urm = H.gap_matrix(300, 400, k, k, long_row=200)
    n_random, n_iter, _ = H.plan(300, 400, k)
    omega = np.random.RandomState(k).normal(size=(300, n_random))
    eng = _engine(urm, k)
    try:
        s1 = eng.pure_svd(omega, n_iter)
        u1, i1 = _factors(eng)
        s2 = eng.pure_svd(omega, n_iter)
        u2, i2 = _factors(eng)
        assert s1.tobytes() == s2.tobytes() and u1.tobytes() == u2.tobytes() and i1.tobytes() == i2.tobytes()
    finally:
        eng.close()


def test_refused_calls_leave_the_factors_unchanged():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = H.case_matrix(40, 30, 1)
    rng = np.random.RandomState(0)
    U0, V0 = rng.rand(40, 3).astype(np.float32), rng.rand(30, 3).astype(np.float32)
    eng = Engine(40, 30, 3, 1, 1, model=L.MODEL_MF)
    try:
        eng.set_tensor(L.T_USER_EMB, U0)
        eng.set_tensor(L.T_ITEM_EMB, V0)
        omega = rng.normal(size=(30, 13))
        with pytest.raises(L.GanmfError, match="has not been called for both sides"):
            eng.pure_svd(omega, 4)
        eng.set_confidence(0, urm)
        with pytest.raises(L.GanmfError, match="has not been called for both sides"):
            eng.pure_svd(omega, 4)
        eng.set_confidence(1, sps.csr_matrix(urm.T))
        for bad, n_iter, match in [(rng.normal(size=(30, 2)), 4, "below num_factors"),
                                   (rng.normal(size=(30, 31)), 4, r"above min\(num_users, num_items\)"),
                                   (omega, -1, "negative")]:
            with pytest.raises(L.GanmfError, match=match) as err:
                eng.pure_svd(bad, n_iter)
            assert "(-1)" in str(err.value)
        for value in (np.nan, np.inf):
            bad = omega.copy()
            bad[7, 5] = value
            with pytest.raises(L.GanmfError, match="not finite"):
                eng.pure_svd(bad, 4)
        u, i = _factors(eng)
        assert u.tobytes() == U0.tobytes() and i.tobytes() == V0.tobytes()
        eng.pure_svd(omega, 4)                                     # the handle is usable as before
        assert np.isfinite(eng.get_tensor(L.T_USER_EMB)).all()
    finally:
        eng.close()
    big = Engine(400, 400, 3, 1, 1, model=L.MODEL_MF)
    try:
        m = sps.identity(400, dtype=np.float32, format="csr")
        big.set_confidence(0, m)
        big.set_confidence(1, m)
        B0, C0 = rng.rand(400, 3).astype(np.float32), rng.rand(400, 3).astype(np.float32)
        big.set_tensor(L.T_USER_EMB, B0)
        big.set_tensor(L.T_ITEM_EMB, C0)
        with pytest.raises(L.GanmfError, match="above the limit of %d" % L.SVD_MAX_RANDOM) as err:
            big.pure_svd(rng.normal(size=(400, L.SVD_MAX_RANDOM + 1)), 4)
        assert "(-1)" in str(err.value)
        u, i = _factors(big)
        assert u.tobytes() == B0.tobytes() and i.tobytes() == C0.tobytes()
    finally:
        big.close()


def test_a_multi_rank_handle_is_refused_with_the_factors_unchanged():
    """rank 0 of a two-rank loopback group (tests/test_gpu_dist_local.py builds such handles on one GPU) with both sides uploaded:
    the entry is a single-GPU one, it would factorise one shard's rows"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = H.case_matrix(40, 30, 1)
    rng = np.random.RandomState(2)
    U0, V0 = rng.rand(40, 3).astype(np.float32), rng.rand(30, 3).astype(np.float32)
    eng = Engine(40, 30, 3, 4, 8, world_size=2, rank=0)
    try:
        eng.comm_init_local(4242)
        eng.set_confidence(0, urm)
        eng.set_confidence(1, sps.csr_matrix(urm.T))
        eng.set_tensor(L.T_USER_EMB, U0)
        eng.set_tensor(L.T_ITEM_EMB, V0)
        with pytest.raises(L.GanmfError, match="single-GPU entry") as err:
            eng.pure_svd(rng.normal(size=(30, 13)), 4)
        assert "(-1)" in str(err.value)
        u, i = _factors(eng)
        assert u.tobytes() == U0.tobytes() and i.tobytes() == V0.tobytes()
    finally:
        eng.close()


def test_a_matrix_of_rank_five_is_reported_and_nothing_is_written():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    rows = np.random.RandomState(0).randint(1, 6, (5, 30)).astype(np.float32)
    urm = sps.csr_matrix(rows[np.arange(40) % 5])
    rng = np.random.RandomState(1)
    U0, V0 = rng.rand(40, 3).astype(np.float32), rng.rand(30, 3).astype(np.float32)
    eng = Engine(40, 30, 3, 1, 1, model=L.MODEL_MF)
    try:
        eng.set_confidence(0, urm)
        eng.set_confidence(1, sps.csr_matrix(urm.T))
        eng.set_tensor(L.T_USER_EMB, U0)
        eng.set_tensor(L.T_ITEM_EMB, V0)
        with pytest.raises(L.GanmfError, match=r"\(-4\).*Cholesky-QR broke down in half step \d+ of \d+ .*pass [12].*fewer factors") as err:
            eng.pure_svd(rng.normal(size=(30, 13)), 4)
        print("puresvd rank-5 message:", err.value)
        u, i = _factors(eng)
        assert u.tobytes() == U0.tobytes() and i.tobytes() == V0.tobytes()
    finally:
        eng.close()


def _counted(model, name):
    got = []
    inner = getattr(model, name)

    def wrapper(*a, **kw):
        got.append(inner(*a, **kw))
        return got[-1]
    setattr(model, name, wrapper)
    return got


def test_fit_end_to_end_against_the_golden_fixture(golden_dir, tmp_path):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from MatrixFactorization.PureSVDRecommender import PureSVDRecommender
    z = np.load(os.path.join(golden_dir, "puresvd_tiny.npz"))
    urm = sps.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(z["shape"]), dtype=np.float32)
    seed, k, u64, i64 = int(z["seed"]), int(z["num_factors"]), z["USER_factors"], z["ITEM_factors"]
    n_random, n_iter, _ = H.plan(40, 30, k)
    np.random.seed(seed)
    omega = np.random.normal(size=(30, n_random))
    u32, i32, _ = H.pure_svd(urm, omega, k, n_iter, np.float32)
    S64 = u64.dot(i64.T)
    h_score = np.abs(u32.astype(np.float64).dot(i32.astype(np.float64).T) - S64).max() / np.abs(S64).max()
    model = PureSVDRecommender(urm)
    np.random.seed(seed)
    model.fit(num_factors=k)
    try:
        user, item = model.USER_factors, model.ITEM_factors
        S = user.astype(np.float64).dot(item.astype(np.float64).T)
        d_score = np.abs(S - S64).max() / np.abs(S64).max()
        print("puresvd parity fit(num_factors=3) vs the sklearn fixture: e_score device %.3e float32 %.3e" % (d_score, h_score))
        assert d_score <= FACTOR * h_score
        sig64 = np.sqrt((i64 * i64).sum(0))
        assert np.abs(model.Sigma - sig64).max() <= FACTOR * h_score * sig64[0]
        # recommend() with seen items removed: the top-5 of the float64 scores wherever those are further apart at the cut than the error
        err = d_score * np.abs(S64).max()
        seen = np.asarray(urm.todense()) != 0
        masked = np.where(seen, -np.inf, S64)
        warm = [u for u in range(40) if urm[u].nnz > 0]
        lists = model.recommend(warm, cutoff=5)
        compared = 0
        for u, got in zip(warm, lists):
            order = np.argsort(-masked[u], kind="stable")
            top = masked[u][order]
            if np.min(top[:5] - top[1:6]) > 2 * err:
                assert list(got) == list(order[:5]), u
                compared += 1
        assert compared >= 10
        assert model.recommend(0, cutoff=5) == []                 # the user without an entry is cold under the MF contract
        # the evaluator and the activity study take the model through the device route
        rng = np.random.RandomState(4)
        test = sps.csr_matrix(((~seen) * (rng.rand(40, 30) < 0.15)) * rng.randint(1, 6, (40, 30)), dtype=np.float32)
        hook = _counted(model, "evaluate_on_device")
        results, _ = EvaluatorHoldoutFast(test, [5]).evaluateRecommender(model)
        assert len(hook) >= 1 and all(r is not None for r in hook)
        assert 0.0 <= results[5]["MAP"] <= 1.0
        study = model.activity_study(test, [3, 10], cutoff=5)
        from MatrixFactorization.IALSRecommender import IALSRecommender
        als = IALSRecommender(urm)
        try:
            als.fit(epochs=1, num_factors=3)
            assert sorted(study.keys()) == sorted(als.activity_study(test, [3, 10], cutoff=5).keys())
        finally:
            als.engine.close()
        # saveModel -> a fresh instance's loadModel -> the same score bytes
        before = model._compute_item_score(warm)
        model.saveModel(str(tmp_path))
        fresh = PureSVDRecommender(urm)
        fresh.loadModel(str(tmp_path))
        try:
            assert fresh._compute_item_score(warm).tobytes() == before.tobytes()
        finally:
            fresh.engine.close()
    finally:
        model.engine.close()
