"""EvaluatorHoldoutFast(full_metrics=True) through the device route (ganmf_evaluate_full: RMSE inside the selection kernel,
per-item counts and the novelty / popularity sums in the metric kernel) against the reference's stored row (KAT-1), the
full-mode host route and the per-user evaluator on the same model."""
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.evaluation import BEYOND_ACCURACY, FULL_METRICS, EvaluatorHoldout, EvaluatorHoldoutFast

pytestmark = pytest.mark.gpu

_SUM_BASED = {"ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "F1", "HIT_RATE", "ARHR"}


def _close(got, want, rtol, what):
    if math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= 1e-15 + rtol * abs(want), (what, got, want)


def _device_rows(ev, model, calls=None):
    """evaluateRecommender with the device route asserted (every block through evaluate_full_on_device)"""
    n = [0]
    orig = model.evaluate_full_on_device

    def counted(*a, **k):
        n[0] += 1
        out = orig(*a, **k)
        assert out is not None
        return out
    model.evaluate_full_on_device = counted
    try:
        res, text = ev.evaluateRecommender(model)
    finally:
        del model.evaluate_full_on_device
    assert n[0] >= 1 and (calls is None or n[0] == calls), n[0]
    return res


def _host_rows(ev, model):
    ev.use_device_metrics = False
    try:
        return ev.evaluateRecommender(model)[0]
    finally:
        ev.use_device_metrics = True


def _compare(dev, ref, cutoffs, acc_rtol, what):
    for c in cutoffs:
        assert list(dev[c]) == list(ref[c]) == list(FULL_METRICS), (what, c)
        for k in FULL_METRICS:
            rtol = 2e-6 if k == "RMSE" else (acc_rtol if k in _SUM_BASED else 1e-12)
            _close(dev[c][k], ref[c][k], rtol, (what, c, k))


def _model(mode, n_users, n_items, k, seed, density=0.08, **kw):
    from ganmf_amd.GANMF import GANMF
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_users, n_items) < density).astype(np.float32)
    m[np.arange(n_users), rng.randint(0, n_items, n_users)] = 1.0
    urm = sps.csr_matrix(m)
    model = GANMF(urm, mode=mode, is_experiment=True, **kw)
    model._build(k, 16, 32)
    model.engine.set_tensor(100, rng.randn(model.num_users, k).astype(np.float32))
    model.engine.set_tensor(101, rng.randn(model.num_items, k).astype(np.float32))
    model.URM_train = model._URM_eval
    return model, urm, rng


def test_kat1_full_row_through_device_route(golden_dir):
    from ganmf_amd.GANMF import GANMF
    t = np.load(os.path.join(golden_dir, "kat1_checkpoint_tensors.npz"))
    exp = json.load(open(os.path.join(golden_dir, "kat1_expected.json")))["expected_metrics"]
    train = sps.load_npz(os.path.join(golden_dir, "LastFM_URM_train.npz")).tocsr()
    test = sps.load_npz(os.path.join(golden_dir, "LastFM_URM_test.npz")).tocsr()
    model = GANMF(train, mode='item', is_experiment=True)
    model._build(1, 133, 32)
    model.engine.set_tensor(100, t["U"])
    model.engine.set_tensor(101, t["V"])
    model.URM_train = model._URM_eval
    res = _device_rows(EvaluatorHoldoutFast(test, [5, 10, 20, 50], full_metrics=True), model)
    for c, d in exp.items():
        row = res[int(c)]
        assert list(row) == list(d)
        for k, v in d.items():
            _close(row[k], v, 1e-9 if k in BEYOND_ACCURACY else 2e-6, (c, k))
    model.engine.close()


@pytest.mark.parametrize("mode", ["user", "item"])
@pytest.mark.parametrize("exclude_seen", [True, False])
def test_device_full_row_equals_host_routes(mode, exclude_seen):
    """four cut-offs, lists shorter than the cut-off, graded ratings, users without test items, seen test items; the
    device row against the full host route (same sums to 1e-12) and the per-user evaluator; then several blocks"""
    model, urm, rng = _model(mode, 300, 23, 6, seed=11, density=0.5)
    nu, ni = urm.shape
    t = (rng.rand(nu, ni) < 0.25) * rng.randint(1, 6, size=(nu, ni))
    t[rng.rand(nu) < 0.1] = 0
    seen = urm.toarray() != 0
    for u in np.flatnonzero(t.sum(axis=1)):        # every evaluated user keeps an unseen test item: RMSE stays finite
        t[u, np.flatnonzero(~seen[u])[0]] = 3
    test = sps.csr_matrix(t.astype(np.float32))
    cut = [1, 5, 10, 20]
    ev = EvaluatorHoldoutFast(test, cut, exclude_seen=exclude_seen, full_metrics=True)
    dev = _device_rows(ev, model, calls=1)
    _compare(dev, _host_rows(ev, model), cut, 1e-12, "host route")
    slow, _ = EvaluatorHoldout(test, cut, exclude_seen=exclude_seen, full_metrics=True).evaluateRecommender(model)
    _compare(dev, slow, cut, 2e-6, "per-user evaluator")
    assert np.isfinite(dev[5]["RMSE"]) and dev[20]["COVERAGE_USER"] > 0 and dev[5]["NOVELTY"] > 0
    again = _device_rows(ev, model, calls=1)
    assert json.dumps(again) == json.dumps(dev)                           # bitwise reproducible
    ev._block_size = 37                                                   # counts and sums added over 8 calls
    _compare(_device_rows(ev, model, calls=-(-len(ev._users) // 37)), dev, cut, 1e-12, "blocks")
    model.engine.close()


@pytest.mark.parametrize("mode", ["user", "item"])
def test_cold_users_mf_contract(mode):
    """MF contract: users without a training interaction score -inf, get empty lists and make RMSE NaN on both routes"""
    from ganmf_amd.GANMF import GANMF
    rng = np.random.RandomState(4)
    n_users, n_items = 80, 40
    m = (rng.rand(n_users, n_items) < 0.1).astype(np.float32)
    m[np.arange(n_users), rng.randint(0, n_items, n_users)] = 1.0
    m[[3, 17], :] = 0.0            # both modes evaluate the rows of this matrix: users 3 and 17 are cold
    urm = sps.csr_matrix(m)
    model = GANMF(urm, mode=mode, is_experiment=True, score_contract="mf")
    model._build(5, 16, 32)
    model.engine.set_tensor(100, rng.randn(model.num_users, 5).astype(np.float32))
    model.engine.set_tensor(101, rng.randn(model.num_items, 5).astype(np.float32))
    model.URM_train = model._URM_eval
    t = ((rng.rand(n_users, n_items) < 0.2) * (m == 0)).astype(np.float32)
    t[[3, 17], :5] = 1.0
    test = sps.csr_matrix(t)
    ev = EvaluatorHoldoutFast(test, [5, 10], full_metrics=True)
    dev = _device_rows(ev, model)
    host = _host_rows(ev, model)
    _compare(dev, host, [5, 10], 1e-12, "host route")
    assert math.isnan(dev[5]["RMSE"]) and dev[5]["COVERAGE_USER"] < 1.0
    model.engine.close()


def test_wide_rows_read_rmse_before_selection():
    """W > 32768: the selection runs in place on the score buffer and overwrites every picked item with -inf, so RMSE must be
    read before it; the test items are each user's best-scored items, all of them picked"""
    model, urm, rng = _model("user", 64, 33000, 4, seed=2, density=0.001)
    scores = model._compute_item_score(np.arange(64))
    scores[urm.nonzero()] = -np.inf
    top = np.argsort(-scores, axis=1, kind="stable")[:, :3]
    t = np.zeros((64, 33000), np.float32)
    t[np.arange(64)[:, None], top] = rng.randint(1, 6, size=(64, 3))
    test = sps.csr_matrix(t)
    ev = EvaluatorHoldoutFast(test, [3, 10], full_metrics=True)
    dev = _device_rows(ev, model)
    _compare(dev, _host_rows(ev, model), [3, 10], 1e-12, "host route")
    assert dev[3]["HIT_RATE"] == 3.0 and np.isfinite(dev[3]["RMSE"])
    model.engine.close()


def test_disganmf_full_row_device_equals_host():
    from ganmf_amd.DisGANMF import DisGANMF
    rng = np.random.RandomState(6)
    urm = sps.csr_matrix((rng.rand(120, 60) < 0.1).astype(np.float32))
    model = DisGANMF(urm, mode="user", seed=3, is_experiment=True)
    model.fit(num_factors=8, d_nodes=16, epochs=2, batch_size=32)
    test = sps.csr_matrix(((rng.rand(120, 60) < 0.15) * rng.randint(1, 6, size=(120, 60))).astype(np.float32))
    ev = EvaluatorHoldoutFast(test, [5, 10], full_metrics=True)
    _compare(_device_rows(ev, model), _host_rows(ev, model), [5, 10], 1e-12, "DisGANMF")
    model.engine.close()


def test_sharded_engine_full_row_equals_single_gpu_twin():
    from ganmf_amd.GANMF import GANMF
    rng = np.random.RandomState(8)
    urm = sps.csr_matrix((rng.rand(150, 70) < 0.1).astype(np.float32))
    sh = GANMF(urm, mode="user", seed=5, is_experiment=True, dist_backend="local", world_size=2)
    sh.fit(num_factors=8, emb_dim=16, epochs=2, batch_size=32)
    assert type(sh.engine).__name__ == "ShardedEngine"
    twin = GANMF(urm, mode="user", is_experiment=True)
    twin._build(8, 16, 32)
    twin.engine.set_tensor(100, sh.engine.get_tensor(100))
    twin.engine.set_tensor(101, sh.engine.get_tensor(101))
    twin.URM_train = twin._URM_eval
    test = sps.csr_matrix(((rng.rand(150, 70) < 0.15) * rng.randint(1, 6, size=(150, 70))).astype(np.float32))
    ev = EvaluatorHoldoutFast(test, [5, 10], full_metrics=True)
    _compare(_device_rows(ev, sh), _device_rows(ev, twin), [5, 10], 1e-12, "sharded vs single")
    sh.engine.close()
    twin.engine.close()


def test_full_entry_points_reject_bad_input():
    from ganmf_amd._lib import GanmfError
    model, urm, rng = _model("user", 40, 30, 4, seed=3)
    eng = model.engine
    test = sps.csr_matrix((rng.rand(40, 30) < 0.2).astype(np.float32))
    test.sort_indices()
    disc, ideal = np.ones(5), np.ones((4, 5))
    eng.set_test(test, np.ones(test.nnz))
    with pytest.raises(GanmfError):       # no ratings yet
        eng.evaluate_full(np.arange(4), [5], disc, ideal)
    with pytest.raises(GanmfError):       # ratings of another length
        eng.set_test_ratings(np.ones(test.nnz + 1))
    eng.set_test_ratings(test.data)
    with pytest.raises(GanmfError):       # no weights yet
        eng.evaluate_full(np.arange(4), [5], disc, ideal)
    eng.set_eval_item_weights(np.ones(29), np.ones(29))
    with pytest.raises(GanmfError):       # weights of another width
        eng.evaluate_full(np.arange(4), [5], disc, ideal)
    eng.set_eval_item_weights(np.ones(30), np.ones(30))
    with pytest.raises(GanmfError):       # more cut-offs than one call takes
        eng.evaluate_full(np.arange(4), list(range(1, 10)), np.ones(9), np.ones((4, 9)))
    sums, counts = eng.evaluate_full(np.arange(4), [5], disc, ideal, remove_seen=False)
    assert sums.shape == (1, 13) and counts.shape == (1, 30) and counts.sum() == 20
    eng.set_test(test, np.ones(test.nnz))  # a new test matrix drops the ratings
    with pytest.raises(GanmfError):
        eng.evaluate_full(np.arange(4), [5], disc, ideal)
    eng.close()
