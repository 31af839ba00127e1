"""WRMF / implicit ALS on the device: ganmf_als_half_sweep against the numpy restatement (tests/helpers_ials.py), determinism, the
factors-only handle, IALSRecommender end to end, and the reference's own logged hyper-parameter search
(experiments/IALSRecommender__1M/results.txt, tests/golden/ials_trial_logs_ml1m.json) as known answers.

Tolerance of every comparison of factors: MEASURED, not fixed.  Per case the device's largest per-row relative error against the
float64 restatement must be at most 4 x the error of the float32 restatement on the same inputs: a different summation order and
Cholesky instead of the reference's inverse are both backward stable with the same k . eps . cond scaling.  Both figures are printed;
their values from the first run on an MI355X are in profiles/ials_parity.md."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_ials as H

pytestmark = pytest.mark.gpu

FACTOR = 4.0


def _profile_matrix(n_rows, n_cols, seed, long_row):
    """[n_rows, n_cols] float ratings in {1 .. 5}: row 0 without an entry, row 1 with one, row 2 with `long_row` (more than one
    gather tile of 32), the others at a density of 12 %"""
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_rows, n_cols) < 0.12) * rng.randint(1, 6, (n_rows, n_cols)).astype(np.float64)
    m[0] = 0
    m[1] = 0
    m[1, n_cols // 2] = 3
    m[2] = 0
    m[2, rng.permutation(n_cols)[:long_row]] = rng.randint(1, 6, long_row)
    return sps.csr_matrix(m.astype(np.float32))


def _sweep_case(n_rows, n_cols, long_row, k, reg, scaling, side):
    """One half sweep of `side` on a handle whose solved side has the rows of _profile_matrix: returns (device X, X0, Y, C, engine)"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    M = _profile_matrix(n_rows, n_cols, 100 + k, long_row)
    alpha, eps = (2.0, 1.0) if scaling == "linear" else (10.0, 0.5)
    C = H.confidence(M, scaling, alpha, eps)                   # rows = the side being solved
    rng = np.random.RandomState(k)
    X0 = rng.rand(n_rows, k).astype(np.float32)
    Y = (k ** -0.5 * rng.rand(n_cols, k)).astype(np.float32)
    n_users, n_items = (n_rows, n_cols) if side == 0 else (n_cols, n_rows)
    eng = Engine(n_users, n_items, k, 1, 1, model=L.MODEL_MF)
    eng.set_confidence(side, C)
    eng.set_tensor(L.T_USER_EMB if side == 0 else L.T_ITEM_EMB, X0)
    eng.set_tensor(L.T_ITEM_EMB if side == 0 else L.T_USER_EMB, Y)
    eng.als_half_sweep(side, reg)
    X = eng.get_tensor(L.T_USER_EMB if side == 0 else L.T_ITEM_EMB)
    return X, X0, Y, C, eng


def _check_against_helper(X, X0, Y, C, reg, label):
    ref = H.half_sweep(X0, Y, C, reg, np.float64)
    f32 = H.half_sweep(X0, Y, C, reg, np.float32)
    e_dev, e_f32 = H.row_error(X, ref), H.row_error(f32, ref)
    print("ials parity %s: device %.3e  float32 restatement %.3e  ratio %.2f" % (label, e_dev, e_f32, e_dev / e_f32 if e_f32 else np.inf))
    assert np.isfinite(X).all()
    assert X[0].tobytes() == X0[0].tobytes(), "a row without a stored entry must come back unchanged"
    assert e_dev <= FACTOR * e_f32, (label, e_dev, e_f32)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("scaling", ["linear", "log"])
@pytest.mark.parametrize("reg", [1e-5, 1e-2])
@pytest.mark.parametrize("k", [1, 7, 32, 33, 64, 65])
def test_half_sweep_against_float64(k, reg, scaling, side):
    X, X0, Y, C, eng = _sweep_case(77, 131, 120, k, reg, scaling, side)
    try:
        _check_against_helper(X, X0, Y, C, reg, "77x131 k=%d reg=%g %s side=%d" % (k, reg, scaling, side))
        # pad columns stay zero: the scoring product reads the factor rows over their padded width
        ids = np.arange(X.shape[0])
        s = eng.scores(ids, transposed=(side == 1))
        want = X.astype(np.float64).dot(Y.astype(np.float64).T)
        bound = (np.abs(X).astype(np.float64).dot(np.abs(Y).astype(np.float64).T)).max()
        assert np.abs(s - want).max() <= 1e-5 * bound
    finally:
        eng.close()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("reg,scaling", [(1e-5, "linear"), (1e-2, "log")])
@pytest.mark.parametrize("k", [250, 256])
def test_half_sweep_against_float64_at_the_largest_ranks(k, reg, scaling, side):
    X, X0, Y, C, eng = _sweep_case(300, 280, 120, k, reg, scaling, side)
    try:
        _check_against_helper(X, X0, Y, C, reg, "300x280 k=%d reg=%g %s side=%d" % (k, reg, scaling, side))
    finally:
        eng.close()


@pytest.mark.parametrize("k", [7, 65])
def test_two_half_sweeps_from_the_same_state_return_the_same_bytes(k):
    from ganmf_amd import _lib as L
    X, X0, Y, C, eng = _sweep_case(77, 131, 120, k, 1e-3, "linear", 0)
    try:
        eng.set_tensor(L.T_USER_EMB, X0)
        eng.als_half_sweep(0, 1e-3)
        again = eng.get_tensor(L.T_USER_EMB)
        assert again.tobytes() == X.tobytes()
        assert eng.get_tensor(L.T_ITEM_EMB).tobytes() == Y.tobytes()      # the fixed side is not written
    finally:
        eng.close()


def test_mf_handle_holds_factors_only():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(9, 11, 3, 1, 1, model=L.MODEL_MF)
    try:
        assert eng.shape(L.T_USER_EMB) == (9, 3) and eng.shape(L.T_ITEM_EMB) == (11, 3)
        with pytest.raises(L.GanmfError, match="unknown tensor"):
            eng.shape(0)
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_MF"):
            eng.train_epoch(np.arange(9))
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_MF"):
            eng.train_step(0, np.arange(1))
        with pytest.raises(L.GanmfError, match="ganmf_als_set_confidence has not been called"):
            eng.als_half_sweep(0, 1e-3)
        with pytest.raises(L.GanmfError, match="side 1 is 11 x 9"):
            eng.set_confidence(1, sps.csr_matrix(np.ones((9, 11), np.float32)))
        # the best slots and the snapshot entries work on it
        U = np.arange(27, dtype=np.float32).reshape(9, 3)
        eng.set_tensor(L.T_USER_EMB, U)
        eng.snapshot_best()
        eng.set_tensor(L.T_USER_EMB, np.zeros((9, 3), np.float32))
        eng.restore_best()
        assert np.array_equal(eng.get_tensor(L.T_USER_EMB), U)
    finally:
        eng.close()
    big = Engine(9, 11, 257, 1, 1, model=L.MODEL_MF)
    try:
        big.set_confidence(0, sps.csr_matrix(np.ones((9, 11), np.float32)))
        with pytest.raises(L.GanmfError, match="above the limit of 256"):
            big.als_half_sweep(0, 1e-3)
    finally:
        big.close()


def test_a_system_that_is_not_positive_definite_is_reported():
    """reg = 0 and item factors of rank 1 at k = 3: the kernel raises its flag, the entry names the first such row and the rows
    keep their factors (no NaN is written)"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(5, 6, 3, 1, 1, model=L.MODEL_MF)
    try:
        m = np.zeros((5, 6), np.float32)
        m[2, 1] = m[2, 4] = m[3, 0] = 2.0
        eng.set_confidence(0, sps.csr_matrix(m))
        U0 = np.full((5, 3), 0.5, np.float32)
        eng.set_tensor(L.T_USER_EMB, U0)
        eng.set_tensor(L.T_ITEM_EMB, np.outer(np.arange(1, 7), [1.0, 0.0, 0.0]).astype(np.float32))
        with pytest.raises(L.GanmfError, match="row 2.*not positive definite"):
            eng.als_half_sweep(0, 0.0)
        assert np.array_equal(eng.get_tensor(L.T_USER_EMB), U0)
        eng.als_half_sweep(0, 1e-3)                              # the handle is usable as before
        assert np.isfinite(eng.get_tensor(L.T_USER_EMB)).all()
    finally:
        eng.close()


def _counted(model, name):
    """wraps model.<name> so that its return values are recorded"""
    got = []
    inner = getattr(model, name)

    def wrapper(*a, **kw):
        got.append(inner(*a, **kw))
        return got[-1]
    setattr(model, name, wrapper)
    return got


def test_fit_end_to_end_on_the_tiny_matrix(golden_dir):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from MatrixFactorization.IALSRecommender import IALSRecommender
    urm = sps.load_npz(os.path.join(golden_dir, "tiny_urm.npz")).tocsr().astype(np.float32)
    rng = np.random.RandomState(4)
    dense = np.asarray(urm.todense())
    dense[5] = 0                                               # a cold user
    test = sps.csr_matrix(((dense == 0) * (rng.rand(*dense.shape) < 0.15)).astype(np.float32))
    test = sps.csr_matrix(test.multiply(rng.randint(1, 6, dense.shape)), dtype=np.float32)
    urm = sps.csr_matrix(dense)
    kw = dict(confidence_scaling="log", alpha=3.0, epsilon=0.7, reg=1e-3)
    model = IALSRecommender(urm)
    np.random.seed(21)
    model.fit(epochs=3, num_factors=8, **kw)
    np.random.seed(21)
    V0 = 8 ** -0.5 * np.random.random_sample((urm.shape[1], 8))
    try:
        U64, V64 = H.fit(urm, V0.astype(np.float32), 3, "log", 3.0, 0.7, 1e-3, np.float64)
        U32, V32 = H.fit(urm, V0.astype(np.float32), 3, "log", 3.0, 0.7, 1e-3, np.float32)
        for name, got, ref, f32 in (("USER", model.USER_factors, U64, U32), ("ITEM", model.ITEM_factors, V64, V32)):
            e_dev, e_f32 = H.row_error(got, ref), H.row_error(f32, ref)
            print("ials parity fit(3 epochs, k=8) %s_factors: device %.3e  float32 restatement %.3e" % (name, e_dev, e_f32))
            assert e_dev <= FACTOR * e_f32, (name, e_dev, e_f32)
        assert model.epochs_best == 2 and np.array_equal(model.USER_factors[5], np.zeros(8, np.float32))
        # the evaluator and the activity study take the model through the device route
        hook = _counted(model, "evaluate_on_device")
        results, _ = EvaluatorHoldoutFast(test, [5]).evaluateRecommender(model)
        assert len(hook) >= 1 and all(r is not None for r in hook)
        assert 0.0 <= results[5]["MAP"] <= 1.0
        groups = _counted(model, "evaluate_groups_on_device")
        study = model.activity_study(test, [3, 10], cutoff=5)
        assert len(groups) >= 1 and all(r is not None for r in groups)
        assert np.nansum(study["n_users"]) > 0
        # a cold user gets an empty list, a warm one a full one of unseen items
        assert model.recommend(5, cutoff=5) == []
        lists = model.recommend([0, 5, 6], cutoff=5)
        assert lists[1] == [] and len(lists[0]) == 5 and not set(lists[0]) & set(urm[0].indices)
        scores = model._compute_item_score([0, 5])
        assert np.isneginf(scores[1]).all()
        assert np.abs(scores[0] - model.USER_factors[0].dot(model.ITEM_factors.T)).max() <= 1e-5 * np.abs(scores[0]).max()
    finally:
        model.engine.close()


# ---- the reference's logged search as known answers: ML-1M small split, five epochs, seed 1234, MAP@5 on the validation split ----
@pytest.fixture(scope="module")
def ml1m(golden_dir):
    logs = json.load(open(os.path.join(golden_dir, "ials_trial_logs_ml1m.json")))
    train = sps.load_npz(os.path.join(golden_dir, "Movielens1M_URM_train_small.npz")).tocsr()
    valid = sps.load_npz(os.path.join(golden_dir, "Movielens1M_URM_validation.npz")).tocsr()
    return logs["trials"], train, valid


def _replay(trial, train, evaluator):
    from MatrixFactorization.IALSRecommender import IALSRecommender
    model = IALSRecommender(train)
    np.random.seed(1234)
    try:
        model.fit(**trial["params"])
        results, _ = evaluator.evaluateRecommender(model)
    finally:
        model.engine.close()
    return float(results[5]["MAP"])


def test_logged_rank_one_and_best_trials(ml1m):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    trials, train, valid = ml1m
    ev = EvaluatorHoldoutFast(valid, [5], exclude_seen=True)
    ones = [t for t in trials if t["params"]["num_factors"] == 1]
    assert len(ones) == 8
    for t in ones:
        got, logged = _replay(t, train, ev), t["validation_at5"]["MAP"]
        print("ials pin k=1 %s alpha=%.4g reg=%.3g: MAP@5 %.5f logged %.5f" % (t["params"]["confidence_scaling"], t["params"]["alpha"],
                                                                                   t["params"]["reg"], got, logged))
        assert abs(got - logged) <= 5e-4, (t["params"], got, logged)
    best = max(trials, key=lambda t: t["validation_at5"]["MAP"])
    assert best["params"]["num_factors"] == 25
    got = _replay(best, train, ev)
    print("ials pin best trial (k=25): MAP@5 %.5f logged %.5f" % (got, best["validation_at5"]["MAP"]))
    assert abs(got - 0.14476) <= 0.005, got


def test_all_logged_trials_replay(ml1m):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    trials, train, valid = ml1m
    ev = EvaluatorHoldoutFast(valid, [5], exclude_seen=True)
    logged = np.array([t["validation_at5"]["MAP"] for t in trials])
    got = np.array([_replay(t, train, ev) for t in trials])
    rank = lambda a: np.argsort(np.argsort(a)).astype(np.float64)      # noqa: E731  (no ties among 50 float MAPs)
    rho = float(np.corrcoef(rank(logged), rank(got))[0, 1])
    print("ials pin 50 trials: Spearman rho %.4f, largest |MAP@5 - logged| %.4f" % (rho, np.abs(got - logged).max()))
    assert rho >= 0.97, rho
    assert np.abs(got - logged).max() <= 0.01, (int(np.abs(got - logged).argmax()), np.abs(got - logged).max())
