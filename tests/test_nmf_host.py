"""NMF on the host, no device: the numpy restatement (tests/helpers_nmf.py) against sklearn's own float32 results recorded in
tests/golden/nmf_tiny.npz (tools/make_nmf_fixture.py; no test imports sklearn), the two initialisations, the coin flip, the two
stopping rules and the random stream of NMFRecommender.fit() driven through a helper engine, and the argument errors.

Restatement against sklearn.  sklearn computes in float32, the restatement here in float64, so the two differ by float32's rounding
of a whole run.  The yardstick for that is measured, as tests/test_gpu_puresvd.py measures its own: the distance of the FLOAT32
restatement from the float64 one, on the same quantity, times 4 (another summation order -- BLAS against Cython loops -- is backward
stable with the same scaling).  Quantities: W . H after the fit's iterations and W_t . H after transform's, as max |difference| over
max |W64 . H64|.  The error scalar is bounded the same way, 4 x the float32 restatement's own distance
from the float64 error; one float32 number's distance can fall far below one rounding by chance, so that yardstick has a floor of
eps32 = 2^-23.  Every figure is printed."""
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_nmf as HN

FACTOR = 4.0
ITERS = (1, 10, 50)
SOLVERS = {"mu_fro": HN.FROBENIUS, "mu_kl": HN.KULLBACK_LEIBLER, "cd": HN.FROBENIUS}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "nmf_tiny.npz"))


def _matrix(fx, c):
    return sps.csr_matrix((fx[c + "/X_data"], fx[c + "/X_indices"], fx[c + "/X_indptr"]), shape=tuple(fx[c + "/shape"]))


def _run(X, W0, H0, tag, n, perms, dtype):
    if tag == "cd":
        W, H, _ = HN.cd(X, W0, H0, perms[:n], True, dtype)
        return W, H
    return HN.mu(X, W0, H0, SOLVERS[tag], n, True, dtype)


def _transform(X, H, tag, n, perms_t, k, dtype):
    if tag == "cd":
        return HN.cd(X, np.zeros((X.shape[0], k)), H, perms_t[:n, None], False, dtype)[0]
    start = np.full((X.shape[0], k), np.sqrt(X.mean() / k), dtype=np.float32)
    return HN.mu(X, start, H, SOLVERS[tag], n, False, dtype)[0]


@pytest.mark.parametrize("tag", sorted(SOLVERS))
@pytest.mark.parametrize("case", ["a", "b"])
def test_float64_restatement_against_sklearn(fx, case, tag):
    X, k = _matrix(fx, case), int(fx[case + "/k"])
    W0, H0 = fx[case + "/random_W0"], fx[case + "/random_H0"]
    perms, perms_t = fx[case + "/perms"], fx[case + "/perms_t"]
    beta = SOLVERS[tag]
    for n in ITERS:
        key = "%s/%s_%d_" % (case, tag, n)
        Wsk, Hsk, err_sk, Wt_sk = fx[key + "W"], fx[key + "H"], float(fx[key + "err"]), fx[key + "Wt"]
        W64, H64 = _run(X, W0, H0, tag, n, perms, np.float64)
        W32, H32 = _run(X, W0, H0, tag, n, perms, np.float32)
        assert W32.dtype == np.float32 and H32.dtype == np.float32
        d_fit, y_fit = HN.product_error(Wsk, Hsk, W64, H64), HN.product_error(W32, H32, W64, H64)
        Wt64 = _transform(X, Hsk, tag, n, perms_t, k, np.float64)
        Wt32 = _transform(X, Hsk, tag, n, perms_t, k, np.float32)
        d_tr, y_tr = HN.product_error(Wt_sk, Hsk, Wt64, Hsk), HN.product_error(Wt32, Hsk, Wt64, Hsk)
        err64 = HN.divergence(X, W64, H64, beta)
        d_err = HN.scalar_error(err_sk, err64)
        b_err = FACTOR * max(HN.scalar_error(HN.divergence(X, W32, H32, beta, np.float32), err64), HN.EPS)
        print("nmf restatement %s n=%d: W.H sklearn-float64 %.3e float32-float64 %.3e ratio %.2f | transform %.3e / %.3e ratio %.2f | "
              "error %.6f sklearn %.6f rel %.3e bound %.3e" % (key, n, d_fit, y_fit, d_fit / y_fit, d_tr, y_tr, d_tr / y_tr, err64,
                                                              err_sk, d_err, b_err))
        assert d_fit <= FACTOR * y_fit, (key, d_fit, y_fit)
        assert d_tr <= FACTOR * y_tr, (key, d_tr, y_tr)
        assert d_err <= b_err, (key, d_err, b_err)
        assert (W64 >= 0).all() and (H64 >= 0).all()


def test_random_init_is_sklearn_s_bit_for_bit(fx):
    from ganmf_amd.NMF import random_init
    for case in "ab":
        X, k, seed = _matrix(fx, case), int(fx[case + "/k"]), int(fx[case + "/seed"])
        np.random.seed(seed)
        W, H = random_init(X, k)
        assert W.dtype == np.float32 and H.dtype == np.float32
        assert np.array_equal(W, fx[case + "/random_W0"]) and np.array_equal(H, fx[case + "/random_H0"])
        # H is drawn first: the stream stands where two standard_normal draws of these sizes leave it
        after = np.random.random_sample()
        np.random.seed(seed)
        np.random.standard_normal(size=(k, X.shape[1]))
        np.random.standard_normal(size=(X.shape[0], k))
        assert after == np.random.random_sample()


def test_nndsvda_split_of_sklearn_s_own_svd(fx):
    from ganmf_amd.NMF import nndsvda_split
    for case in "ab":
        X = _matrix(fx, case)
        W, H = nndsvda_split(fx[case + "/svd_U"], fx[case + "/svd_S"], fx[case + "/svd_V"], X.mean())
        Wsk, Hsk = fx[case + "/nndsvda_W0"], fx[case + "/nndsvda_H0"]
        assert W.dtype == np.float32 and H.dtype == np.float32
        mean = np.float32(X.mean())
        # the same entries were filled with the mean, every other one agrees to float32 rounding
        assert np.array_equal(W == mean, Wsk == mean) and np.array_equal(H == mean, Hsk == mean)
        np.testing.assert_allclose(W, Wsk, rtol=4 * HN.EPS, atol=0)
        np.testing.assert_allclose(H, Hsk, rtol=4 * HN.EPS, atol=0)
        assert (W > 0).all() and (H > 0).all()


def test_nndsvda_picks_the_negative_pair_on_a_tie_and_fills_zeros():
    from ganmf_amd.NMF import nndsvda_split
    U = np.array([[0.5, 0.5], [0.5, -0.5], [0.5, 0.5], [0.5, -0.5]], dtype=np.float32)
    V = np.array([[0.6, 0.8], [0.6, -0.6]], dtype=np.float32)      # column 1: |x_p| |y_p| == |x_n| |y_n| -> the negative pair
    S = np.array([4.0, 1.0], dtype=np.float32)
    W, H = nndsvda_split(U, S, V, 0.25)
    assert np.allclose(W[:, 0], 1.0) and np.allclose(H[0], [1.2, 1.6])
    assert W[0, 1] == 0.25 and W[2, 1] == 0.25 and W[1, 1] > 0.25 and H[1, 0] == 0.25 and H[1, 1] > 0.25


def _model(urm, errors=None, violations=None):
    from ganmf_amd.NMF import NMFRecommender
    model = NMFRecommender(urm)
    model._make_engine = lambda k: HN.NMFHelperEngine(model.n_users, model.n_items, k, errors=errors, violations=violations)
    return model


def _urm():
    return HN.case_matrix(40, 30, 5)


def test_the_coin_flip_consumes_exactly_one_draw_and_switches_one_of_the_two():
    from ganmf_amd.NMF import random_init
    seen = set()
    for seed in range(8):
        np.random.seed(seed)
        coin = int(np.random.binomial(1, 0.5, 1)[0])
        W0, H0 = random_init(_urm(), 3)
        model = _model(_urm(), errors=[10.0, 9.9999] + [5.0, 4.99999], violations=[0.0, 0.0])
        np.random.seed(seed)
        model.fit(num_factors=3, solver="coordinate_descent", beta_loss="kullback-leibler")
        kinds = [c[0] for c in model.engine.calls]
        if coin:      # the solver became the multiplicative update, the loss stayed
            assert "cd" not in kinds and all(c[1] == HN.KULLBACK_LEIBLER for c in model.engine.calls)
        else:         # the loss became Frobenius, the solver stayed
            assert "mu" not in kinds and all(c[1] == HN.FROBENIUS for c in model.engine.calls if c[0] == "error")
        seen.add(coin)
        # the start is what sklearn draws BEHIND one binomial draw
        assert model.engine.first_W is not None and np.array_equal(model.engine.first_W, W0)
    assert seen == {0, 1}


def test_mu_stops_at_iteration_ten():
    model = _model(_urm(), errors=[100.0, 99.995, 50.0, 49.999])      # init, check 1: (100 - 99.995) / 100 < 1e-4; transform alike
    model.fit(num_factors=3)
    assert model.n_iter_ == 10 and model.reconstruction_err_ == 99.995 and model.transform_n_iter_ == 10
    assert model.engine.calls == [("error", 0), ("mu", 0, 10, True, True), ("error", 0), ("mu", 0, 10, False, True)]


def test_mu_compares_with_the_previous_check_relative_to_the_initial_error():
    # 100 -> 90 -> 89.5 -> 89.495: (89.5 - 89.495) / 100 = 5e-5 < tol stops the third check, where / 89.5 would as well but
    # (90 - 89.5) / 100 = 5e-3 does not stop the second
    model = _model(_urm(), errors=[100.0, 90.0, 89.5, 89.495, 7.0, 6.0, 5.9999])
    model.fit(num_factors=3, beta_loss="kullback-leibler")
    assert model.n_iter_ == 30 and model.reconstruction_err_ == 89.495 and model.transform_n_iter_ == 20
    assert [c[2] for c in model.engine.calls if c[0] == "mu"] == [10] * 5
    assert all(c[1] == 1 for c in model.engine.calls)


def test_mu_runs_to_five_hundred_iterations():
    fit_errors = [1000.0 - i for i in range(51)]           # init + 50 checks, each 1e-3 of the initial error below the last
    model = _model(_urm(), errors=fit_errors + [10.0, 9.99999])
    model.fit(num_factors=3)
    assert model.n_iter_ == 500 and model.reconstruction_err_ == fit_errors[-1] and model.transform_n_iter_ == 10
    assert sum(c[2] for c in model.engine.calls if c[0] == "mu" and c[3]) == 500


def test_mu_with_an_initial_error_of_zero_carries_on_as_numpy_does():
    """0 / 0 is nan in sklearn's numpy arithmetic, nan < tol is False: no ZeroDivisionError, the loop runs to max_iter"""
    model = _model(_urm(), errors=[0.0] * 51 + [0.0] * 51)
    model.fit(num_factors=3)
    assert model.n_iter_ == 500 and model.transform_n_iter_ == 500 and model.reconstruction_err_ == 0.0


def test_cd_stops_by_the_ratio_to_the_first_violation_and_leaves_the_stream_where_sklearn_does():
    k = 3
    model = _model(_urm(), violations=[50.0, 1.0, 0.004, 8.0, 0.0004])      # 0.004 / 50 <= 1e-4 in iteration 3; transform in 2
    np.random.seed(21)
    model.fit(num_factors=k, solver="coordinate_descent")
    after = np.random.random_sample()
    assert model.n_iter_ == 3 and model.transform_n_iter_ == 2
    np.random.seed(21)
    np.random.standard_normal(size=(k, 30))
    np.random.standard_normal(size=(40, k))
    want = [np.random.permutation(k) for _ in range(2 * 3 + 2)]      # two per fit iteration, one per transform iteration, no more
    assert after == np.random.random_sample()
    cd_calls = [c for c in model.engine.calls if c[0] == "cd"]
    got = [p for c in cd_calls for p in c[1].reshape(-1, k)]
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert [c[2] for c in cd_calls] == [True] * 3 + [False] * 2
    # the transform solve starts from zeros, the multiplicative one from sqrt(mean / k)
    assert not model.engine.transform_start.any()


def test_cd_with_a_first_violation_of_zero_stops_at_once():
    model = _model(_urm(), violations=[0.0, 0.0])
    model.fit(num_factors=3, solver="coordinate_descent")
    assert model.n_iter_ == 1 and model.transform_n_iter_ == 1


def test_cd_runs_to_five_hundred_iterations():
    model = _model(_urm(), violations=[10.0] * 500 + [1.0, 0.0])
    model.fit(num_factors=3, solver="coordinate_descent")
    assert model.n_iter_ == 500 and model.transform_n_iter_ == 2


def test_fit_through_the_float64_engine_matches_the_restatement_and_snapshots():
    """the whole of fit() on the helper engine: USER_factors are transform's W, ITEM_factors the fit's H"""
    urm = _urm()
    model = _model(urm)
    np.random.seed(3)
    model.fit(num_factors=3)
    from ganmf_amd.NMF import random_init
    np.random.seed(3)
    W0, H0 = random_init(urm, 3)
    W, H = HN.mu(urm, W0, H0, HN.FROBENIUS, model.n_iter_, True)
    assert np.allclose(model.ITEM_factors, H.T, rtol=1e-6)
    assert model.reconstruction_err_ == pytest.approx(HN.divergence(urm, W, H, HN.FROBENIUS), rel=1e-12)
    Wt, _ = HN.mu(urm, np.full((40, 3), np.sqrt(urm.mean() / 3), dtype=np.float32), H, HN.FROBENIUS, model.transform_n_iter_, False)
    assert np.allclose(model.USER_factors, Wt, rtol=1e-6)
    assert not np.allclose(model.USER_factors, W, rtol=1e-3)      # a second solve, not the W of the fit
    assert np.allclose(model.engine.best[100], Wt) and model.n_iter_ % 10 == 0 and 10 <= model.n_iter_ <= 500


def test_nndsvda_start_through_the_float64_svd(fx):
    """_initial_factors with the helper's float64 pure_svd against sklearn's own start: every entry further than 1e-7 from the 1e-6
    threshold agrees, and those left out are at most 1 % (the fixture's matrices keep sklearn itself inside that)"""
    for case in "ab":
        X, k, seed = _matrix(fx, case), int(fx[case + "/k"]), int(fx[case + "/seed"])
        model = _model(X)
        model._build(k)
        model.engine.set_confidence(0, X)
        model.engine.set_confidence(1, sps.csr_matrix(X.T))
        np.random.seed(seed)
        W, H = model._initial_factors(X, k, "nndsvda")
        for got, want in ((W, fx[case + "/nndsvda_W0"]), (H, fx[case + "/nndsvda_H0"])):
            near = np.abs(np.minimum(got, want).astype(np.float64) - 1e-6) <= 1e-7
            assert near.mean() <= 0.01
            np.testing.assert_allclose(got[~near], want[~near], rtol=0, atol=2e-4 * want.max())


@pytest.mark.parametrize("kwargs,exc,match", [
    (dict(l1_ratio=1.5), AssertionError, "l1_ratio must be between 0 and 1, provided value was 1.5"),
    (dict(solver="als"), ValueError, "Value for 'solver' not recognized. Acceptable values are .*provided was 'als'"),
    (dict(init_type="nndsvd"), ValueError, r"Value for 'init_type' not recognized. Acceptable values are \['random', 'nndsvda'\], provided was 'nndsvd'"),
    (dict(beta_loss="itakura-saito"), ValueError, "Value for 'beta_loss' not recognized. Acceptable values are .*provided was 'itakura-saito'"),
    (dict(num_factors=0), ValueError, r"num_factors must be in \[1, 270\]"),
    (dict(num_factors=271), ValueError, r"num_factors must be in \[1, 270\]"),
    (dict(num_factors=31, init_type="nndsvda"), ValueError, "can only be used when n_components <= min"),
    (dict(num_factors=25, init_type="nndsvda"), ValueError, r"draws num_factors \+ 10 = 35 random vectors"),
])
def test_argument_errors_need_no_device(kwargs, exc, match):
    from ganmf_amd.NMF import NMFRecommender
    model = NMFRecommender(_urm())
    state = np.random.get_state()[1].copy()
    with pytest.raises(exc, match=match):
        model.fit(**kwargs)
    assert model.engine is None and np.array_equal(np.random.get_state()[1], state)      # nothing built, nothing drawn
