"""full_metrics=True: the reference's whole 19-metric row from both evaluators (the per-user EvaluatorHoldout and the host
route of EvaluatorHoldoutFast), against outputs of the reference's own Base/Evaluation/Evaluator.py, CPU only."""
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.base import BaseRecommender
from ganmf_amd.evaluation import BEYOND_ACCURACY, FULL_METRICS, EvaluatorHoldout, EvaluatorHoldoutFast


class _Factors(BaseRecommender):
    def __init__(self, urm, U, V, cold=()):
        super().__init__(urm)
        self.U, self.V, self.cold = U, V, np.asarray(cold, dtype=np.int64)

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        scores = self.U[user_id_array] @ self.V.T
        scores[np.isin(np.asarray(user_id_array), self.cold)] = -np.inf
        return scores


def _close(got, want, rtol, what):
    if isinstance(want, float) and math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= 1e-15 + rtol * abs(want), (what, got, want)


def _check_row(res, exp, acc_rtol, what):
    for c, d in exp.items():
        row = res[int(c)]
        assert list(row) == list(d) == list(FULL_METRICS), (what, c, list(row))
        for k, v in d.items():
            _close(row[k], v, 1e-9 if k in BEYOND_ACCURACY else acc_rtol, (what, c, k))


def _hetrec(golden_dir):
    f = np.load(os.path.join(golden_dir, "evaluator_factors.npz"))
    train = sps.load_npz(os.path.join(golden_dir, "hetrec2011_URM_train_small.npz")).tocsr()
    val = sps.load_npz(os.path.join(golden_dir, "hetrec2011_URM_validation.npz")).tocsr()
    return _Factors(train, f["U"], f["V"]), val, json.load(open(os.path.join(golden_dir, "evaluator_expected.json")))


def test_full_row_matches_reference_golden(golden_dir):
    rec, val, exp = _hetrec(golden_dir)
    res, text = EvaluatorHoldout(val, [5, 10], full_metrics=True).evaluateRecommender(rec)
    _check_row(res, exp, 2e-6, "slow")
    assert "SHANNON_ENTROPY: " in text and text.index("RMSE") < text.index("NOVELTY")
    ev = EvaluatorHoldoutFast(val, [5, 10], full_metrics=True)
    ev._block_size = 700                                         # four blocks: counts and sums added across them
    fast, _ = ev.evaluateRecommender(rec)
    _check_row(fast, exp, 2e-5, "fast host route")
    for c in (5, 10):
        assert np.isfinite(fast[c]["RMSE"])
        for k in BEYOND_ACCURACY:
            _close(fast[c][k], res[c][k], 1e-12, ("fast vs slow", c, k))


def test_kat1_full_row_on_cpu(golden_dir):
    t = np.load(os.path.join(golden_dir, "kat1_checkpoint_tensors.npz"))
    exp = json.load(open(os.path.join(golden_dir, "kat1_expected.json")))["expected_metrics"]
    train = sps.load_npz(os.path.join(golden_dir, "LastFM_URM_train.npz")).tocsr()
    test = sps.load_npz(os.path.join(golden_dir, "LastFM_URM_test.npz")).tocsr()
    rec = _Factors(train, t["V"], t["U"])       # item mode: evaluation users are the generator's items
    res, _ = EvaluatorHoldout(test, [5, 10, 20, 50], full_metrics=True).evaluateRecommender(rec)
    _check_row(res, exp, 2e-6, "slow")
    fast, _ = EvaluatorHoldoutFast(test, [5, 10, 20, 50], full_metrics=True).evaluateRecommender(rec)
    _check_row(fast, exp, 2e-6, "fast host route")


def _edge(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "evaluator_edge_expected.json")))
    train, test = sps.csr_matrix(np.array(g["train"], np.float32)), sps.csr_matrix(np.array(g["test"], np.float32))
    rec = _Factors(train, np.array(g["U"], np.float32), np.array(g["V"], np.float32), cold=[g["cold_user"]])
    return rec, test, g


@pytest.mark.parametrize("block", [None, 3])
def test_edge_fixture_both_evaluators(golden_dir, block):
    """short lists, an empty list (cold user: RMSE NaN as in the reference), graded ratings, a recommended item without
    training interactions, users without test items, a seen test item"""
    rec, test, g = _edge(golden_dir)
    cut = g["cutoffs"]
    res, _ = EvaluatorHoldout(test, cut, full_metrics=True).evaluateRecommender(rec)
    _check_row(res, g["expected"], 2e-6, "slow")
    ev = EvaluatorHoldoutFast(test, cut, full_metrics=True)
    ev._block_size = block
    fast, _ = ev.evaluateRecommender(rec)
    _check_row(fast, g["expected"], 2e-6, "fast")
    assert g["expected"]["8"]["COVERAGE_USER"] < 1.0 and math.isnan(g["expected"]["8"]["RMSE"])


def test_fast_full_host_route_matches_slow_evaluator():
    """random case with finite RMSE: the two evaluators key for key, the new values to 1e-12"""
    rng = np.random.RandomState(5)
    n_users, n_items = 60, 15
    train = (rng.rand(n_users, n_items) < 0.5).astype(np.float32)
    train[:6, :] = 1.0
    train[:6, :3] = 0.0
    test = ((rng.rand(n_users, n_items) < 0.3) * rng.randint(1, 6, size=(n_users, n_items)) * (train == 0)).astype(np.float32)
    test[7, np.flatnonzero(train[7])[0]] = 4.0      # seen and in the test set (the user keeps unseen test items)
    test[7, np.flatnonzero(train[7] == 0)[0]] = 2.0
    rec = _Factors(sps.csr_matrix(train), rng.randn(n_users, 4).astype(np.float32), rng.randn(n_items, 4).astype(np.float32))
    test = sps.csr_matrix(test)
    slow, _ = EvaluatorHoldout(test, [1, 5, 8], full_metrics=True).evaluateRecommender(rec)
    ev = EvaluatorHoldoutFast(test, [1, 5, 8], full_metrics=True)
    ev._block_size = 7
    fast, _ = ev.evaluateRecommender(rec)
    for c in (1, 5, 8):
        assert list(fast[c]) == list(slow[c]) == list(FULL_METRICS)
        assert np.isfinite(fast[c]["RMSE"])
        for k, v in slow[c].items():
            _close(fast[c][k], v, 1e-12 if k in BEYOND_ACCURACY else 2e-6, (c, k))


def test_default_rows_unchanged():
    """without full_metrics the keys and the fast evaluator's NaN RMSE stay as they were"""
    rng = np.random.RandomState(1)
    train = sps.csr_matrix((rng.rand(20, 10) < 0.3).astype(np.float32))
    test = sps.csr_matrix((rng.rand(20, 10) < 0.3).astype(np.float32))
    rec = _Factors(train, rng.randn(20, 3).astype(np.float32), rng.randn(10, 3).astype(np.float32))
    slow, _ = EvaluatorHoldout(test, [5]).evaluateRecommender(rec)
    fast, _ = EvaluatorHoldoutFast(test, [5]).evaluateRecommender(rec)
    assert not set(BEYOND_ACCURACY) & (set(slow[5]) | set(fast[5]))
    assert np.isnan(fast[5]["RMSE"])


def test_early_stopping_on_coverage_item():
    """EarlyStoppingScheduler watching a beyond-accuracy metric through a full-metrics evaluator"""
    from ganmf_amd.early_stopping import EarlyStoppingScheduler
    rng = np.random.RandomState(3)
    n_users, n_items = 30, 20
    train = sps.csr_matrix((rng.rand(n_users, n_items) < 0.2).astype(np.float32))
    test = sps.csr_matrix((rng.rand(n_users, n_items) < 0.3).astype(np.float32))
    U = rng.randn(n_users, 4).astype(np.float32)
    diverse = rng.randn(n_items, 4).astype(np.float32)
    popular = np.zeros((n_items, 4), np.float32)
    popular[:, 0] = np.linspace(2, 1, n_items)                 # every user gets (about) the same items
    popular_u = np.abs(U)

    class M(_Factors):
        saved = loaded = stopped = 0

        def save_current_model(self):
            self.saved += 1

        def load_model(self):
            self.loaded += 1

        def stop_fit(self):
            self.stopped += 1

    m = M(train, popular_u, popular)
    ev = EvaluatorHoldoutFast(test, [5, 10], full_metrics=True)
    es = EarlyStoppingScheduler(m, ev, metrics=["COVERAGE_ITEM"], freq=1, allow_worse=0, after=0)
    seen = []
    for ep, (u, v) in enumerate([(popular_u, popular), (U, diverse), (popular_u, popular)], start=1):
        m.U, m.V = u, v
        seen.append(ev.evaluateRecommender(m)[0][5]["COVERAGE_ITEM"])
        es(ep)
    assert seen[1] > seen[0] and seen[2] < seen[1]
    assert [s[0] for s in es.get_scores()] == seen
    assert (m.saved, m.stopped, m.loaded) == (2, 1, 1)
