"""EvaluatorNegativeItemSample / EvaluatorNegativeItemSampleFast (host routes, CPU only) against the stored output of the
reference's own Base/Evaluation/Evaluator.py:419-590 (tools/make_negative_sample_golden.py): an item in both the test and the
negative matrix, a user without negatives, a user whose candidates are all seen (RMSE NaN), a user with two candidates, users
below minRatingsPerUser, graded ratings, a seen test item."""
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.base import BaseRecommender
from ganmf_amd.evaluation import (BEYOND_ACCURACY, FULL_METRICS, EvaluatorHoldoutFast, EvaluatorNegativeItemSample,
                                  EvaluatorNegativeItemSampleFast)


class _Factors(BaseRecommender):
    """MF contract: items outside items_to_compute score -inf (Base/BaseMatrixFactorizationRecommender.py:113-119)"""

    def __init__(self, urm, U, V):
        super().__init__(urm)
        self.U, self.V = U, V

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        if items_to_compute is None:
            return self.U[user_id_array] @ self.V.T
        scores = np.full((len(user_id_array), self.V.shape[0]), -np.inf, dtype=np.float32)
        scores[:, items_to_compute] = self.U[user_id_array] @ self.V[items_to_compute].T
        return scores


class _FactorsWithBlocks(_Factors):
    """the same recommender with the block-wise candidate API the Fast class prefers"""
    calls = 0

    def recommend_candidates(self, user_id_array, candidates_csr, cutoff, remove_seen_flag=True, candidates_key=None):
        self.calls += 1
        self.keys = getattr(self, "keys", set()) | {candidates_key}
        out = np.full((len(user_id_array), cutoff), -1, dtype=np.int32)
        for i, u in enumerate(user_id_array):
            items = candidates_csr.indices[candidates_csr.indptr[u]:candidates_csr.indptr[u + 1]]
            got = self.recommend(np.atleast_1d(u), cutoff=cutoff, remove_seen_flag=remove_seen_flag, items_to_compute=items)[0]
            out[i, :len(got)] = got
        return out


def _close(got, want, rtol, what):
    if isinstance(want, float) and math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= 1e-15 + rtol * abs(want), (what, got, want)


def _check_row(res, exp, acc_rtol, what, keys=FULL_METRICS):
    for c, d in exp.items():
        row = res[int(c)]
        if keys is FULL_METRICS:
            assert list(row) == list(FULL_METRICS), (what, c, list(row))     # the reference's key order
        else:
            assert set(row) == set(FULL_METRICS[:11]), (what, c, list(row))  # the default eleven-value row
        for k in keys:
            _close(row[k], d[k], 1e-9 if k in BEYOND_ACCURACY else acc_rtol, (what, c, k))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "negative_sample_expected.json")))
    g["train"] = sps.csr_matrix(np.array(g["train"], np.float32))
    g["test"] = sps.csr_matrix(np.array(g["test"], np.float32))
    g["negative"] = sps.csr_matrix(np.array(g["negative"], np.float32))
    g["U"], g["V"] = np.array(g["U"], np.float32), np.array(g["V"], np.float32)
    return g


def _rec(g, cls=_Factors):
    return cls(g["train"], g["U"], g["V"])


def test_reference_order_class_matches_golden(golden):
    g = golden
    ev = EvaluatorNegativeItemSample(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"],
                                     full_metrics=True)
    assert ev.EVALUATOR_NAME == "EvaluatorNegativeItemSample"
    res, text = ev.evaluateRecommender(_rec(g))
    _check_row(res, g["expected"], 2e-6, "reference order")
    assert math.isnan(g["expected"]["5"]["RMSE"]) and "CUTOFF: 5 - ROC_AUC: " in text
    eleven, _ = EvaluatorNegativeItemSample(g["test"], g["negative"], g["cutoffs"],
                                            minRatingsPerUser=g["min_ratings_per_user"]).evaluateRecommender(_rec(g))
    _check_row(eleven, g["expected"], 2e-6, "reference order, default row", keys=FULL_METRICS[:11])


def test_items_to_rank_is_the_reference_construction(golden):
    g = golden
    for cls in (EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast):
        m = cls(g["test"], g["negative"], g["cutoffs"]).URM_items_to_rank
        assert m.indptr.tolist() == g["items_to_rank"]["indptr"] and m.indices.tolist() == g["items_to_rank"]["indices"]
        assert np.all(m.data == 1)
        u = g["both_user"]
        both = np.intersect1d(g["test"][u].indices, g["negative"][u].indices)
        assert len(both) == 1                                            # stored in both matrices, ranked once
        row = m.indices[m.indptr[u]:m.indptr[u + 1]]
        assert len(row) == len(np.unique(row)) == g["test"][u].nnz + g["negative"][u].nnz - 1


@pytest.mark.parametrize("cls", [_Factors, _FactorsWithBlocks])
@pytest.mark.parametrize("block", [None, 5])
def test_fast_class_matches_golden(golden, cls, block):
    """per-user route and block-wise route; `block` = 5 forces four blocks, whose sums and counts are added"""
    g = golden
    rec = _rec(g, cls)
    ev = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"],
                                         full_metrics=True)
    ev._block_size = block
    res, _ = ev.evaluateRecommender(rec)
    _check_row(res, g["expected"], 2e-5, "fast, full row")
    ev9 = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"])
    ev9._block_size = block
    res9, _ = ev9.evaluateRecommender(rec)
    assert all(math.isnan(res9[c]["RMSE"]) for c in g["cutoffs"])
    _check_row(res9, g["expected"], 2e-5, "fast, default row", keys=[k for k in FULL_METRICS[:11] if k != "RMSE"])
    if cls is _FactorsWithBlocks:
        assert rec.calls == (1 if block is None else 4)                  # the nine-metric rows went through recommend_candidates
        assert rec.keys == {ev9._device_token}                           # one token per evaluator: one upload of its candidates
        for c in g["cutoffs"]:
            for k in FULL_METRICS[:11]:
                if k != "RMSE":
                    _close(res9[c][k], res[c][k], 1e-12, ("blocks vs users", c, k))


def test_fast_blocks_equal_one_block(golden):
    g = golden
    rows = []
    for block in (None, 1, 7):
        ev = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"],
                                             full_metrics=True)
        ev._block_size = block
        rows.append(ev.evaluateRecommender(_rec(g))[0])
    for other in rows[1:]:
        for c in g["cutoffs"]:
            for k in FULL_METRICS:
                _close(other[c][k], rows[0][c][k], 1e-12, (c, k))


def test_recommender_that_ignores_items_to_compute_is_ranked_full_width(golden):
    """the reference's GANMF contract: items_to_compute ignored -> both classes rank the whole catalogue, the Fast class as
    EvaluatorHoldoutFast does"""
    g = golden

    class Ignores(_Factors):
        honours_items_to_compute = False

        def _compute_item_score(self, user_id_array, items_to_compute=None):
            return self.U[user_id_array] @ self.V.T

    rec = Ignores(g["train"], g["U"], g["V"])
    kw = dict(minRatingsPerUser=g["min_ratings_per_user"], full_metrics=True)
    fast, _ = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], **kw).evaluateRecommender(rec)
    hold, _ = EvaluatorHoldoutFast(g["test"], g["cutoffs"], **kw).evaluateRecommender(rec)
    assert json.dumps(fast) == json.dumps(hold)
    slow, _ = EvaluatorNegativeItemSample(g["test"], g["negative"], g["cutoffs"], **kw).evaluateRecommender(rec)
    for c in g["cutoffs"]:
        for k in FULL_METRICS:
            _close(fast[c][k], slow[c][k], 1e-12 if k in BEYOND_ACCURACY else 2e-5, (c, k))


def test_block_route_over_its_limits_falls_back_to_the_per_user_route(golden):
    """a recommender whose block-wise API refuses the call (a cut-off or a candidate list over its limits) is evaluated user by
    user from then on, with the same result, for the nine-metric rows as for the full row"""
    g = golden

    class Refuses(_Factors):
        calls = 0

        def recommend_candidates(self, user_id_array, candidates_csr, cutoff, remove_seen_flag=True, candidates_key=None):
            self.calls += 1
            raise RuntimeError("a row has more candidates than one call takes")

    rec = Refuses(g["train"], g["U"], g["V"])
    ev = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"])
    ev._block_size = 5
    res, _ = ev.evaluateRecommender(rec)
    assert rec.calls == 1                                                # asked once, not once per block
    plain = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"])
    plain._block_size = 5
    assert json.dumps(res) == json.dumps(plain.evaluateRecommender(_rec(g))[0])
