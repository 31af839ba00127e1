"""PureSVD on the host (no GPU): the numpy restatement of the device's algorithm (tests/helpers_puresvd.py) in float64 against
sklearn.utils.extmath.randomized_svd itself and against the golden fixture, and PureSVDRecommender's host logic -- sklearn's choice of
n_random / n_iter / orientation, the draw from numpy's global stream, argument checks, persistence -- over a helper engine."""
import json
import os
import zipfile

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_puresvd as H

SKLEARN_CASES = [(40, 30, 1), (40, 30, 3), (257, 131, 13), (131, 257, 13), (300, 200, 8), (200, 300, 8), (500, 400, 45)]


@pytest.mark.parametrize("n_users,n_items,k", SKLEARN_CASES)
def test_helper_in_float64_equals_sklearn(n_users, n_items, k):
    extmath = pytest.importorskip("sklearn.utils.extmath")
    urm = sps.csr_matrix(H.case_matrix(n_users, n_items, 3 + k), dtype=np.float64)
    n_random, n_iter, transposed = H.plan(n_users, n_items, k)
    seed = 100 + k
    np.random.seed(seed)
    u, s, vt = extmath.randomized_svd(urm, n_components=k, random_state=None)
    ref_user, ref_item = u, (s[:, None] * vt).T
    np.random.seed(seed)
    omega = np.random.normal(size=(min(n_users, n_items), n_random))
    user, item, sigma = H.pure_svd(urm, omega, k, n_iter, np.float64)
    S, Sref = user.dot(item.T), ref_user.dot(ref_item.T)
    e_score = np.abs(S - Sref).max() / np.abs(Sref).max()
    e_sigma = np.abs(sigma - s).max() / s[0]
    e_user = np.abs(H.align_signs(user, ref_user) - ref_user).max(axis=0)
    print("puresvd helper vs sklearn %dx%d k=%d n_iter=%d: score %.2e sigma %.2e USER columns %.2e" % (
        n_users, n_items, k, n_iter, e_score, e_sigma, e_user.max()))
    assert e_score <= 1e-10 and e_sigma <= 1e-10
    assert (e_user <= 1e-6).all()
    assert np.array_equal(np.sign(user[np.abs(user).argmax(0), np.arange(k)]), np.ones(k))      # the sign rule itself
    assert np.abs(user - ref_user).max() <= 1e-6                                                # and it is sklearn's


def test_plan_is_sklearn_s_on_both_sides_of_its_rules():
    from ganmf_amd.PureSVD import svd_plan
    assert svd_plan(300, 200, 19) == (29, 7, False)
    assert svd_plan(300, 200, 20) == (30, 4, False)          # 20 < 0.1 * 200 is false
    assert svd_plan(40, 30, 3) == (13, 4, False)             # 0.1 * 30 == 3.0 in floating point
    assert svd_plan(257, 131, 13) == (23, 7, False)          # 13 < 13.100000000000001
    assert svd_plan(200, 300, 19) == (29, 7, True)
    assert svd_plan(200, 200, 5) == (15, 7, False)           # a square matrix is not transposed
    for args in [(300, 200, 19), (40, 30, 3), (131, 257, 13)]:
        assert svd_plan(*args) == H.plan(*args)


def _golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "puresvd_tiny.npz"))
    urm = sps.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(z["shape"]))
    return urm, int(z["seed"]), int(z["num_factors"]), z["USER_factors"], z["ITEM_factors"]


def test_helper_reproduces_the_golden_fixture(golden_dir):
    urm, seed, k, ref_user, ref_item = _golden(golden_dir)
    assert urm.shape == (40, 30) and urm[0].nnz == 0 and urm[:, 1].nnz == 0 and urm[2].nnz == 1
    n_random, n_iter, _ = H.plan(40, 30, k)
    np.random.seed(seed)
    user, item, _ = H.pure_svd(urm, np.random.normal(size=(30, n_random)), k, n_iter, np.float64)
    Sref = ref_user.dot(ref_item.T)
    assert np.abs(user.dot(item.T) - Sref).max() <= 1e-10 * np.abs(Sref).max()
    assert np.abs(user - ref_user).max() <= 1e-6
    assert not user[0].any() and not item[1].any()


def test_a_matrix_of_low_rank_is_reported_by_the_helper():
    rows = np.random.RandomState(0).randint(1, 6, (5, 30)).astype(np.float64)
    urm = sps.csr_matrix(rows[np.arange(40) % 5])
    with pytest.raises(H.Breakdown, match="half step 0"):
        H.pure_svd(urm, np.random.RandomState(1).normal(size=(30, 13)), 3, 4, np.float32)


def _model(urm, **kw):
    from ganmf_amd.PureSVD import PureSVDRecommender
    model = PureSVDRecommender(urm, **kw)
    model._make_engine = lambda k: H.SVDHelperEngine(model.n_users, model.n_items, k)
    return model


@pytest.mark.parametrize("n_users,n_items,k,n_iter", [(60, 50, 4, 7), (60, 50, 5, 4), (50, 60, 4, 7), (50, 60, 5, 4)])
def test_fit_calls_the_engine_as_sklearn_would(n_users, n_items, k, n_iter):
    urm = H.case_matrix(n_users, n_items, 5)
    model = _model(urm)
    np.random.seed(3)
    model.fit(num_factors=k)
    assert model.engine.calls == [((min(n_users, n_items), k + 10), n_iter)]
    assert (model.engine.conf[0] != urm).nnz == 0 and model.engine.conf[0].dtype == np.float32
    assert model.USER_factors.shape == (n_users, k) and model.ITEM_factors.shape == (n_items, k)
    assert model.Sigma.shape == (k,) and (np.diff(model.Sigma) <= 0).all() and model.Sigma[-1] > 0
    # the draw is numpy's global stream: the same seed gives the same factors, and what follows the draw in the stream is what follows
    # min(shape) * (k + 10) normal deviates
    first = model.USER_factors.copy()
    after = np.random.random_sample()
    np.random.seed(3)
    model.fit(num_factors=k)
    assert np.array_equal(model.USER_factors, first)
    np.random.seed(3)
    np.random.normal(size=(min(n_users, n_items), k + 10))
    assert np.random.random_sample() == after
    np.random.seed(4)
    model.fit(num_factors=k)
    assert not np.array_equal(model.USER_factors, first)
    # and the result is the factorisation: sklearn's accuracy statement, loosely -- the scores approach the best rank-k approximation
    dense = np.asarray(urm.todense(), dtype=np.float64)
    u, s, vt = np.linalg.svd(dense, full_matrices=False)
    assert np.abs(model.Sigma - s[:k]).max() <= 2e-2 * s[0]


def test_fit_signature_and_argument_checks():
    import inspect
    from ganmf_amd import _lib as L
    from ganmf_amd.PureSVD import PureSVDRecommender
    sig = inspect.signature(PureSVDRecommender.fit)
    assert [(n, p.default) for n, p in sig.parameters.items() if n != "self"] == [("num_factors", 100)]
    assert PureSVDRecommender.RECOMMENDER_NAME == "PureSVDRecommender"
    assert PureSVDRecommender.mode == "user" and PureSVDRecommender.score_contract == "mf"
    assert L.SVD_MAX_RANDOM >= 266
    model = _model(H.case_matrix(60, 50, 5))
    with pytest.raises(ValueError, match="more than min"):
        model.fit(num_factors=41)
    with pytest.raises(ValueError, match="at least 1"):
        model.fit(num_factors=0)
    wide = _model(sps.csr_matrix((400, 400), dtype=np.float32))
    with pytest.raises(ValueError, match="SVD_MAX_RANDOM"):
        wide.fit(num_factors=L.SVD_MAX_RANDOM - 9)
    with pytest.raises(RuntimeError, match="no device state"):
        model.USER_factors
    with pytest.raises(RuntimeError, match="no device state"):
        model.saveModel("/nonexistent")


def test_save_and_load_in_the_reference_s_zip_layout(tmp_path):
    urm = H.case_matrix(60, 50, 5)
    model = _model(urm)
    np.random.seed(9)
    model.fit(num_factors=4)
    model.saveModel(str(tmp_path))
    path = os.path.join(str(tmp_path), "PureSVDRecommender.zip")
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
        kinds = json.loads(z.read("__DataIO_attribute_to_type_dict.json").decode())
        files = json.loads(z.read("__DataIO_attribute_to_file_name.json").decode())
    assert names == {"USER_factors.npy", "ITEM_factors.npy", "_cold_user_mask.npy", "use_bias.json",
                     "__DataIO_attribute_to_type_dict.json", "__DataIO_attribute_to_file_name.json"}
    assert kinds["USER_factors"] == "np.ndarray" and kinds["use_bias"] == "json" and files["ITEM_factors"] == "ITEM_factors.npy"
    fresh = _model(urm)
    fresh.loadModel(str(tmp_path))
    assert np.array_equal(fresh.USER_factors, model.USER_factors) and np.array_equal(fresh.ITEM_factors, model.ITEM_factors)
    model.saveModel(str(tmp_path), file_name="other")
    assert os.path.exists(os.path.join(str(tmp_path), "other.zip"))
    with pytest.raises(ValueError, match="saved factors"):
        _model(H.case_matrix(61, 50, 5)).loadModel(str(tmp_path))


def test_factors_wider_than_fit_can_compute_still_load(tmp_path):
    """MAX_FACTORS is the factorisation's limit (num_factors + 10 random vectors): a saved model above it loads and scores"""
    from ganmf_amd import _lib as L
    urm = H.case_matrix(60, 50, 5)
    k = L.SVD_MAX_RANDOM + 20
    wide = _model(urm)
    with pytest.raises(ValueError, match="random vectors"):
        wide._build(k)
    wide._build(k, limit=False)
    rng = np.random.RandomState(0)
    wide.engine.set_tensor(L.T_USER_EMB, rng.rand(60, k))
    wide.engine.set_tensor(L.T_ITEM_EMB, rng.rand(50, k))
    wide.saveModel(str(tmp_path))
    fresh = _model(urm)
    fresh.loadModel(str(tmp_path))
    assert fresh.num_factors == k and np.array_equal(fresh.ITEM_factors, wide.ITEM_factors)
