"""IALSRecommender's host side without a device: the numpy restatement the GPU tests compare against, the fit loop with its early
stopping, persistence and argument checks.  The engine is tests/helpers_ials.py HelperEngine (float64)."""
import json
import os
import zipfile

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_ials as H


def _urm(n_users=23, n_items=31, density=0.3, seed=0):
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_users, n_items) < density) * rng.randint(1, 6, (n_users, n_items))
    m[4] = 0                                                  # a cold user
    m[:, 7] = 0                                               # a cold item
    return sps.csr_matrix(m.astype(np.float32))


def test_restatement_equals_dense_weighted_least_squares():
    """half_sweep (which uses the Y^T Y shortcut and an inverse) against the stacked least-squares problem over ALL items with
    c = 1, p = 0 where nothing is stored: 23 x 31, k = 5, float64"""
    urm = _urm()
    rng = np.random.RandomState(1)
    k, reg = 5, 1e-3
    Y = rng.rand(31, k) * k ** -0.5
    X0 = rng.rand(23, k)
    for scaling, alpha, eps in (("linear", 2.0, 1.0), ("log", 10.0, 0.5)):
        C = H.confidence(urm, scaling, alpha, eps)
        X = H.half_sweep(X0, Y, C, reg)
        dense_c = np.asarray(C.todense(), dtype=np.float64)
        stored = np.asarray(urm.todense()) != 0
        dense_c[~stored] = 1.0
        for u in range(23):
            if not stored[u].any():
                assert np.array_equal(X[u], X0[u])            # rows without a stored entry are not touched
                continue
            want = H.dense_wls_row(Y, dense_c[u], stored[u].astype(np.float64), reg)
            assert np.abs(X[u] - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), u
    # and the other side is the same routine on the transpose
    Ct = H.confidence(urm, "linear", 2.0).T.tocsr()
    Yi = H.half_sweep(Y, X, Ct, reg)
    assert np.array_equal(Yi[7], Y[7])
    want = H.dense_wls_row(X, np.where(stored[:, 0], np.asarray(Ct.todense())[0], 1.0), stored[:, 0].astype(np.float64), reg)
    assert np.abs(Yi[0] - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("n_rows", [34, 36])
def test_edge_matrix_has_the_stated_rows(n_rows):
    M = H.edge_matrix(n_rows, 260, 3)
    assert M.shape == (n_rows, 260) and M.dtype == np.float32
    want = [0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 0, 0, 0, 0, 0, 200, 0, 0, 1, 1, 0, 0, 200, 5, 5, 5, 5, 5, 64, 0, 33, 200, 5]
    want += [7, 7] * (n_rows == 36)
    assert np.diff(M.indptr).tolist() == want == H.edge_lengths(n_rows)
    assert H.EDGE_TWIN_ROWS == (24, 25, 26, 27, 28, 33)
    assert set(np.unique(M.data)) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    rows = [(M.indices[M.indptr[u]:M.indptr[u + 1]], M.data[M.indptr[u]:M.indptr[u + 1]]) for u in range(n_rows)]
    for u, (cols, _) in enumerate(rows):
        assert len(set(cols.tolist())) == len(cols), u          # no repeated column
        assert cols.size == 0 or (0 <= cols.min() and cols.max() < 260)
    for u in H.EDGE_TWIN_ROWS:
        assert np.array_equal(rows[u][0], rows[24][0]) and np.array_equal(rows[u][1], rows[24][1])
    # only the twins are copies: two other rows of one length are drawn one by one
    assert not np.array_equal(rows[16][0], rows[23][0])
    # the same seed gives the same matrix, another seed another one
    again, other = H.edge_matrix(n_rows, 260, 3), H.edge_matrix(n_rows, 260, 4)
    assert np.array_equal(again.indices, M.indices) and np.array_equal(again.data, M.data)
    assert not np.array_equal(other.indices, M.indices)
    with pytest.raises(ValueError):
        H.edge_matrix(35)


@pytest.mark.parametrize("k,reg,scaling", [(8, 1e-5, "linear"), (40, 1e-2, "log"), (97, 1e-2, "linear")])
def test_cholesky_restatement_equals_the_inverse_restatement(k, reg, scaling):
    """float64, 36 x 260: two algorithms behind the same B and b"""
    alpha, eps = (2.0, 1.0) if scaling == "linear" else (10.0, 0.5)
    C = H.confidence(H.edge_matrix(36, 260, 5), scaling, alpha, eps)
    rng = np.random.RandomState(k)
    X0 = rng.rand(36, k)
    Y = k ** -0.5 * rng.rand(260, k)
    a, b = H.half_sweep(X0, Y, C, reg, np.float64), H.half_sweep_cholesky(X0, Y, C, reg, np.float64)
    assert b.dtype == np.float64
    assert H.row_error(b, a) <= 1e-10
    assert np.array_equal(H.row_errors(b, a).max(), H.row_error(b, a))
    empty = np.flatnonzero(np.diff(C.indptr) == 0)
    assert empty.size == 11 and np.array_equal(b[empty], X0[empty])
    # in float32 it computes in float32: close to float64, not equal to it
    c = H.half_sweep_cholesky(X0, Y, C, reg, np.float32)
    assert c.dtype == np.float32 and 0 < H.row_error(c, a) < 1e-2
    # system_matrix is the B and b both solve
    B, rhs = H.system_matrix(Y, C, 16, reg)
    assert np.abs(B.dot(a[16]) - rhs).max() <= 1e-10 * np.abs(rhs).max()
    with pytest.raises(np.linalg.LinAlgError):
        H.half_sweep_cholesky(X0, Y, C, -1e3, np.float64)


class _ScriptedEvaluator(object):
    """returns the next value of `values` as MAP at cut-off 5 and records the item factors it was shown"""

    def __init__(self, values):
        self.values, self.seen = list(values), []

    def evaluateRecommender(self, model):
        self.seen.append(model.engine.t[101].copy())
        v = self.values[len(self.seen) - 1]
        return {5: {"MAP": v}, 10: {"MAP": -1.0}}, "MAP %f" % v


def _model(urm):
    from ganmf_amd.IALS import IALSRecommender
    model = IALSRecommender(urm)
    model._make_engine = lambda k: H.HelperEngine(model.n_users, model.n_items, k)
    return model


def test_fit_without_evaluator_keeps_the_last_model():
    urm = _urm()
    model = _model(urm)
    np.random.seed(7)
    model.fit(epochs=3, num_factors=4, alpha=2.0, reg=1e-2)
    np.random.seed(7)
    V0 = 4 ** -0.5 * np.random.random_sample((31, 4))
    U, V = H.fit(urm, V0, 3, "linear", 2.0, 1.0, 1e-2)
    assert model.engine.sweeps == 6
    assert np.array_equal(model.USER_factors, U.astype(np.float32))
    assert np.array_equal(model.ITEM_factors, V.astype(np.float32))
    assert np.array_equal(model.USER_factors[4], np.zeros(4, np.float32))      # the cold user stays zero
    assert model.epochs_best == 2                              # the reference's count without validation: the last epoch's index
    assert model.get_early_stopping_final_epochs_dict() == {"epochs": 2}
    assert model.best_validation_metric is None
    assert model.engine.mask_cold is True                      # MF contract
    assert model.RECOMMENDER_NAME == "IALSRecommender" and model.score_contract == "mf" and model.mode == "user"


def test_fit_with_validation_keeps_the_best_model():
    urm = _urm()
    model = _model(urm)
    ev = _ScriptedEvaluator([0.1, 0.3, 0.2, 0.25])
    np.random.seed(3)
    model.fit(epochs=8, num_factors=3, validation_every_n=2, validation_metric="MAP", evaluator_object=ev)
    assert len(ev.seen) == 4 and model.engine.sweeps == 16     # no early stop: all epochs ran
    assert model.epochs_best == 4 and model.best_validation_metric == 0.3
    assert np.array_equal(model.engine.t[101], ev.seen[1])     # the factors of the best validation, not the last ones
    assert not np.array_equal(ev.seen[1], ev.seen[3])
    np.random.seed(3)
    V0 = 3 ** -0.5 * np.random.random_sample((31, 3))
    assert np.array_equal(model.ITEM_factors, H.fit(urm, V0, 4)[1].astype(np.float32))


def test_fit_stops_after_lower_validations_allowed():
    urm = _urm()
    model = _model(urm)
    ev = _ScriptedEvaluator([0.3, 0.2, 0.3, 0.1, 0.9, 0.9])
    model.fit(epochs=12, num_factors=3, validation_every_n=2, validation_metric="MAP", evaluator_object=ev, stop_on_validation=True,
              lower_validations_allowed=3, epochs_min=0)
    # 0.3 (best), then 0.2, 0.3 (not better: the comparison is strict), 0.1: three worse in a row -> stop after epoch 8
    assert len(ev.seen) == 4 and model.engine.sweeps == 16
    assert model.epochs_best == 2 and model.best_validation_metric == 0.3
    assert np.array_equal(model.engine.t[101], ev.seen[0])
    # epochs_min holds the stop back: with epochs_min = 9 the validation at epoch index 9 is the first that may stop
    model = _model(urm)
    ev = _ScriptedEvaluator([0.3, 0.2, 0.3, 0.1, 0.05, 0.9])
    model.fit(epochs=12, num_factors=3, validation_every_n=2, validation_metric="MAP", evaluator_object=ev, stop_on_validation=True,
              lower_validations_allowed=3, epochs_min=9)
    assert len(ev.seen) == 5 and model.epochs_best == 2
    # an evaluator that is never reached leaves the initial factors as the best ones, as the reference does
    model = _model(urm)
    np.random.seed(5)
    model.fit(epochs=2, num_factors=3, validation_every_n=5, validation_metric="MAP", evaluator_object=_ScriptedEvaluator([]))
    np.random.seed(5)
    assert np.array_equal(model.ITEM_factors, (3 ** -0.5 * np.random.random_sample((31, 3))).astype(np.float32))
    assert model.epochs_best == 0


def test_inconsistent_early_stopping_arguments():
    model = _model(_urm())
    with pytest.raises(ValueError, match="Inconsistent"):
        model.fit(epochs=2, num_factors=3, evaluator_object=_ScriptedEvaluator([0.1]))
    with pytest.raises(ValueError, match="Inconsistent"):
        model.fit(epochs=2, num_factors=3, evaluator_object=_ScriptedEvaluator([0.1]), validation_every_n=1, validation_metric="MAP",
                  stop_on_validation=True)
    with pytest.raises(ValueError, match="epochs_max"):
        model.fit(epochs=0, num_factors=3)


def test_argument_errors_need_no_device():
    from ganmf_amd.IALS import IALSRecommender
    model = IALSRecommender(_urm())
    with pytest.raises(ValueError, match="confidence_scaling"):
        model.fit(epochs=1, confidence_scaling="sqrt")
    with pytest.raises(ValueError, match="num_factors"):
        model.fit(epochs=1, num_factors=257)
    with pytest.raises(ValueError, match="num_factors"):
        model.fit(epochs=1, num_factors=0)
    with pytest.raises(RuntimeError, match="no device state"):
        model.USER_factors
    with pytest.raises(RuntimeError, match="no device state"):
        model.recommend([0], cutoff=5)


def test_confidence_is_float32():
    from ganmf_amd.IALS import IALSRecommender
    urm = _urm()
    model = IALSRecommender(urm)
    for scaling, alpha, eps in (("linear", 0.35638532009582496, 1.0), ("log", 16.52147849576996, 0.3007384777107247)):
        C = model._confidence(scaling, alpha, eps)
        assert C.dtype == np.float32 and np.array_equal(C.indices, model.URM_train.indices)
        assert np.array_equal(C.data, H.confidence(urm, scaling, alpha, eps).data)
        r = model.URM_train.data.astype(np.float64)
        want = 1 + alpha * r if scaling == "linear" else 1 + alpha * np.log(1 + r / eps)
        assert np.abs(C.data - want).max() <= 2e-7 * want.max()


def test_save_and_load_use_the_reference_layout(tmp_path):
    urm = _urm()
    model = _model(urm)
    np.random.seed(11)
    model.fit(epochs=2, num_factors=4)
    U, V = model.USER_factors, model.ITEM_factors
    model.saveModel(str(tmp_path))
    path = os.path.join(str(tmp_path), "IALSRecommender.zip")
    with zipfile.ZipFile(path) as z:
        assert sorted(z.namelist()) == sorted(["USER_factors.npy", "ITEM_factors.npy", "_cold_user_mask.npy", "use_bias.json",
                                               "__DataIO_attribute_to_type_dict.json", "__DataIO_attribute_to_file_name.json"])
        kinds = json.loads(z.read("__DataIO_attribute_to_type_dict.json").decode())
        files = json.loads(z.read("__DataIO_attribute_to_file_name.json").decode())
        assert json.loads(z.read("use_bias.json").decode()) is False
    assert kinds == {"USER_factors": "np.ndarray", "ITEM_factors": "np.ndarray", "_cold_user_mask": "np.ndarray", "use_bias": "json"}
    assert files == {"USER_factors": "USER_factors.npy", "ITEM_factors": "ITEM_factors.npy", "_cold_user_mask": "_cold_user_mask.npy",
                     "use_bias": "use_bias.json"}
    other = _model(urm)
    other.loadModel(str(tmp_path))
    assert other.num_factors == 4
    assert other.USER_factors.tobytes() == U.tobytes() and other.ITEM_factors.tobytes() == V.tobytes()
    model.saveModel(str(tmp_path), file_name="named")
    assert os.path.exists(os.path.join(str(tmp_path), "named.zip"))
    with pytest.raises(ValueError, match="saved factors"):
        _model(_urm(n_users=24)).loadModel(str(tmp_path))


def test_trial_log_fixture(golden_dir):
    logs = json.load(open(os.path.join(golden_dir, "ials_trial_logs_ml1m.json")))
    trials = logs["trials"]
    assert len(trials) == 50 and logs["metric"] == "MAP" and logs["at"] == 5
    assert sum(t["params"]["num_factors"] == 1 for t in trials) == 8
    best = max(trials, key=lambda t: t["validation_at5"]["MAP"])
    assert best["params"]["num_factors"] == 25 and abs(best["validation_at5"]["MAP"] - 0.14476) < 1e-5
    from ganmf_amd import tune
    dims = {d.name: d for d in tune.search_space("IALSRecommender", 6040, 3706)}
    assert sorted(dims) == ["alpha", "confidence_scaling", "epsilon", "num_factors", "reg"]
    assert (dims["num_factors"].low, dims["num_factors"].high) == (1, 250)
    assert dims["confidence_scaling"].choices == ["linear", "log"]
    for name, lo, hi in (("alpha", 1e-3, 50.0), ("reg", 1e-5, 1e-2), ("epsilon", 1e-3, 10.0)):
        assert (dims[name].low, dims[name].high, dims[name].prior) == (lo, hi, "log-uniform")
    for t in trials:                                           # every logged trial lies inside the search space
        p = t["params"]
        assert 1 <= p["num_factors"] <= 250 and p["confidence_scaling"] in ("linear", "log") and p["epochs"] == 5
        for name in ("alpha", "reg", "epsilon"):
            assert dims[name].low * (1 - 1e-9) <= p[name] <= dims[name].high * (1 + 1e-9)
