"""diversity_object / ignore_items / ignore_users of the four evaluators on the CPU: the per-user classes and the host routes of
the Fast classes around a plain factor recommender, against rows recorded from the reference's own evaluators
(tools/make_golden_ignore.py -> tests/golden/evaluator_ignore_*)."""
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.base import BaseRecommender
from ganmf_amd.evaluation import (BEYOND_ACCURACY, FULL_METRICS, METRICS, DiversitySimilarity, EvaluatorHoldout, EvaluatorHoldoutFast,
                                  EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast, beyond_accuracy_metrics, list_diversity)

DIV = "DIVERSITY_SIMILARITY"
FULL_WITH_DIV = FULL_METRICS[:FULL_METRICS.index("AVERAGE_POPULARITY") + 1] + (DIV,) + FULL_METRICS[FULL_METRICS.index("AVERAGE_POPULARITY") + 1:]


class _Factors(BaseRecommender):
    """U[ids] @ V.T in float32; `items_to_compute` masks every other item (the MF contract)"""

    def __init__(self, urm, U, V):
        super().__init__(urm)
        self.U, self.V = U, V

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        scores = self.U[user_id_array] @ self.V.T
        if items_to_compute is not None:
            masked = np.full_like(scores, -np.inf)
            masked[:, items_to_compute] = scores[:, items_to_compute]
            scores = masked
        return scores


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "evaluator_ignore_inputs.npz"))
    g = json.load(open(os.path.join(golden_dir, "evaluator_ignore_expected.json")))
    out = dict(rec=_Factors(sps.csr_matrix(z["train"].astype(np.float32)), z["U"], z["V"]),
               test=sps.csr_matrix(z["test"].astype(np.float32)), negative=sps.csr_matrix(z["negative"].astype(np.float32)),
               D=z["D"].astype(np.float64) / 256.0, ignore_items=z["ignore_items"], ignore_users=z["ignore_users"],
               cutoffs=g["cutoffs"], min_ratings=g["min_ratings_per_user"], expected=g["expected"])
    return out


def _close(got, want, rtol, what):
    if isinstance(want, float) and math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= 1e-15 + rtol * abs(want), (what, got, want)


def _check_row(res, exp, acc_rtol, what):
    for c, d in exp.items():
        row = res[int(c)]
        assert list(row) == list(d), (what, c, list(row))
        for k, v in d.items():
            _close(row[k], v, 1e-9 if k in BEYOND_ACCURACY or k == DIV else acc_rtol, (what, c, k))


def _kwargs(fx, name):
    kw = {}
    if name in ("holdout_all", "holdout_diversity", "negative_users_diversity"):
        kw["diversity_object"] = fx["D"]
    if name in ("holdout_all", "holdout_ignore_items"):
        kw["ignore_items"] = fx["ignore_items"]
    if name in ("holdout_all", "holdout_ignore_users", "negative_users_diversity"):
        kw["ignore_users"] = fx["ignore_users"]
    return kw


@pytest.mark.parametrize("name", ["holdout_all", "holdout_diversity", "holdout_ignore_items", "holdout_ignore_users"])
def test_holdout_rows_match_reference(fx, name):
    kw = _kwargs(fx, name)
    exp = fx["expected"][name]
    assert list(exp["5"]) == list(FULL_WITH_DIV if "diversity_object" in kw else FULL_METRICS)
    slow, _ = EvaluatorHoldout(fx["test"], fx["cutoffs"], minRatingsPerUser=fx["min_ratings"], full_metrics=True, **kw).evaluateRecommender(fx["rec"])
    _check_row(slow, exp, 2e-6, name + " slow")
    ev = EvaluatorHoldoutFast(fx["test"], fx["cutoffs"], minRatingsPerUser=fx["min_ratings"], full_metrics=True, **kw)
    ev._block_size = 37
    fast, _ = ev.evaluateRecommender(fx["rec"])
    _check_row(fast, exp, 2e-5, name + " fast host route")
    for c in fx["cutoffs"]:
        for k in BEYOND_ACCURACY + ((DIV,) if "diversity_object" in kw else ()):
            _close(fast[c][k], slow[c][k], 1e-12, ("fast vs slow", c, k))
    assert not fx["rec"].items_to_ignore_flag and len(fx["rec"].items_to_ignore_ID) == 0


def test_negative_sample_rows_match_reference(fx):
    kw = _kwargs(fx, "negative_users_diversity")
    exp = fx["expected"]["negative_users_diversity"]
    args = (fx["test"], fx["negative"], fx["cutoffs"])
    slow, _ = EvaluatorNegativeItemSample(*args, minRatingsPerUser=fx["min_ratings"], full_metrics=True, **kw).evaluateRecommender(fx["rec"])
    _check_row(slow, exp, 2e-6, "negative slow")
    ev = EvaluatorNegativeItemSampleFast(*args, minRatingsPerUser=fx["min_ratings"], full_metrics=True, **kw)
    ev._block_size = 50
    fast, _ = ev.evaluateRecommender(fx["rec"])
    _check_row(fast, exp, 2e-5, "negative fast")
    for c in fx["cutoffs"]:
        for k in BEYOND_ACCURACY + (DIV,):
            _close(fast[c][k], slow[c][k], 1e-12, ("fast vs slow", c, k))


def test_negative_sample_ignores_items_for_every_user(fx):
    """the deliberate deviation from Evaluator.py:530: no evaluated user is ever recommended an ignored item"""
    ignore = fx["ignore_items"]
    for cls in (EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast):
        ev = cls(fx["test"], fx["negative"], [20], minRatingsPerUser=fx["min_ratings"], full_metrics=True, ignore_items=ignore,
                 diversity_object=fx["D"])
        seen = []
        recommend = fx["rec"].recommend

        def spy(*a, **kw):
            out = recommend(*a, **kw)
            seen.extend(out[0] if kw.get("return_scores") else out)
            assert kw["remove_CustomItems_flag"] is True
            return out
        fx["rec"].recommend = spy
        try:
            res, _ = ev.evaluateRecommender(fx["rec"])
        finally:
            del fx["rec"].recommend
        assert len(seen) == len(ev.usersToEvaluate) and not set(np.concatenate([np.asarray(l, dtype=np.int64) for l in seen]).tolist()) & set(ignore.tolist())
        assert res[20]["COVERAGE_ITEM"] > 0 and not fx["rec"].items_to_ignore_flag


def test_key_order_and_presence(fx):
    rec, test = fx["rec"], fx["test"]
    for cls in (EvaluatorHoldout, EvaluatorHoldoutFast):
        plain, _ = cls(test, [5]).evaluateRecommender(rec)
        with_div, _ = cls(test, [5], diversity_object=fx["D"]).evaluateRecommender(rec)
        assert DIV not in plain[5] and set(plain[5]) == set(METRICS)
        assert list(with_div[5]) == list(plain[5]) + [DIV]                     # appended to the eleven
        full, _ = cls(test, [5], full_metrics=True).evaluateRecommender(rec)
        full_div, _ = cls(test, [5], full_metrics=True, diversity_object=fx["D"]).evaluateRecommender(rec)
        assert list(full[5]) == list(FULL_METRICS) and list(full_div[5]) == list(FULL_WITH_DIV)
        assert full_div[5][DIV] == with_div[5][DIV]
    # an object with the reference's attribute is taken like the plain array
    obj = DiversitySimilarity(fx["D"])
    a, _ = EvaluatorHoldoutFast(test, [5], diversity_object=obj).evaluateRecommender(rec)
    assert a[5][DIV] == with_div[5][DIV]
    text = EvaluatorHoldoutFast(test, [5], diversity_object=obj).evaluateRecommender(rec)[1]
    assert "DIVERSITY_SIMILARITY: " in text


def test_ignore_users_are_removed_in_ascending_order(fx):
    ev = EvaluatorHoldoutFast(fx["test"], [5], minRatingsPerUser=fx["min_ratings"], ignore_users=fx["ignore_users"])
    users = np.asarray(ev.usersToEvaluate)
    assert not set(users.tolist()) & set(fx["ignore_users"].tolist()) and np.all(np.diff(users) > 0)
    n_ratings = np.ediff1d(fx["test"].indptr)
    assert len(users) == (n_ratings >= fx["min_ratings"]).sum() - 15          # two of the 17 were below the minimum anyway
    assert np.array_equal(ev._users, users) and ev._ideal_cum.shape[0] == len(users) == len(ev._n_test)


def test_reset_runs_when_the_recommender_raises(fx):
    class Broken(_Factors):
        def _compute_item_score(self, user_id_array, items_to_compute=None):
            assert self.items_to_ignore_flag and len(self.items_to_ignore_ID) == 23
            raise RuntimeError("scores")
    rec = Broken(fx["rec"].URM_train, fx["rec"].U, fx["rec"].V)
    for ev in (EvaluatorHoldout(fx["test"], [5], ignore_items=fx["ignore_items"]),
               EvaluatorHoldoutFast(fx["test"], [5], ignore_items=fx["ignore_items"]),
               EvaluatorNegativeItemSample(fx["test"], fx["negative"], [5], ignore_items=fx["ignore_items"]),
               EvaluatorNegativeItemSampleFast(fx["test"], fx["negative"], [5], ignore_items=fx["ignore_items"])):
        with pytest.raises(RuntimeError, match="scores"):
            ev.evaluateRecommender(rec)
        assert not rec.items_to_ignore_flag and len(rec.items_to_ignore_ID) == 0
        with pytest.raises(RuntimeError, match="scores"):
            ev.evaluateRecommenderByGroup(rec, np.zeros(fx["test"].shape[0], dtype=np.int64))
        assert not rec.items_to_ignore_flag


def test_grouped_rows_respect_the_ignore_lists(fx):
    groups = np.arange(fx["test"].shape[0]) % 3
    kw = dict(minRatingsPerUser=fx["min_ratings"], ignore_items=fx["ignore_items"], ignore_users=fx["ignore_users"])
    slow = EvaluatorHoldout(fx["test"], [5, 20], **kw).evaluateRecommenderByGroup(fx["rec"], groups)
    fast, per_user, users = EvaluatorHoldoutFast(fx["test"], [5, 20], **kw).evaluateRecommenderByGroup(fx["rec"], groups, return_per_user=True)
    plain = EvaluatorHoldout(fx["test"], [5, 20], minRatingsPerUser=fx["min_ratings"]).evaluateRecommenderByGroup(fx["rec"], groups)
    assert not set(users.tolist()) & set(fx["ignore_users"].tolist())
    assert sum(fast[g]["n_users"] for g in range(3)) == len(users) < sum(plain[g]["n_users"] for g in range(3))
    for g in range(3):
        for c in (5, 20):
            for k, v in slow[g][c].items():
                _close(fast[g][c][k], v, 1e-12, (g, c, k))
    assert any(slow[g][20]["MAP"] != plain[g][20]["MAP"] for g in range(3))


def test_diversity_matrix_range_is_asserted(fx):
    bad = fx["D"].copy()
    bad[3, 4] = 1.5
    with pytest.raises(AssertionError):
        EvaluatorHoldout(fx["test"], [5], diversity_object=bad)
    bad[3, 4] = -0.25
    with pytest.raises(AssertionError):
        EvaluatorHoldoutFast(fx["test"], [5], diversity_object=bad)
    with pytest.raises(AssertionError):
        DiversitySimilarity(bad)
    with pytest.raises(ValueError):
        EvaluatorHoldout(fx["test"], [5], diversity_object=fx["D"][:-1, :-1])


def test_diversity_matrix_is_rounded_to_float32_once():
    rng = np.random.RandomState(0)
    D = rng.rand(9, 9)
    ev = EvaluatorHoldout(sps.csr_matrix(np.eye(9, dtype=np.float32)), [4], diversity_object=D)
    assert ev._diversity.dtype == np.float32 and np.array_equal(ev._diversity, D.astype(np.float32))


def test_list_diversity_definition():
    """the skipped last row, the asymmetry, L_c = min(c, len) and the L < 2 rule, against the reference's loop written out"""
    rng = np.random.RandomState(4)
    D = (rng.randint(0, 257, size=(12, 12)) / 256.0).astype(np.float32)
    lists = np.array([[3, 7, 1, 9, 0, 5], [4, 2, 8, -1, -1, -1], [6, -1, -1, -1, -1, -1], [-1] * 6])
    cutoffs = [2, 4, 6, 1]
    got = list_diversity(D, lists, cutoffs)
    for r, row in enumerate(lists):
        ids = row[row >= 0]
        for ci, c in enumerate(cutoffs):
            l = ids[:c]
            want = 0.0
            if len(l) >= 2:
                total = 0.0
                for i in range(len(l) - 1):
                    total += sum(float(D[l[i], l[j]]) for j in range(len(l)) if j != i)
                want = total / (len(l) * (len(l) - 1))
            assert got[r, ci] == pytest.approx(want, rel=1e-15, abs=0), (r, c)
    assert got[0, 0] == float(D[3, 7]) / 2 and D[3, 7] != D[7, 3]
    assert np.all(got[2] == 0.0) and np.all(got[3] == 0.0) and np.all(got[:, 3] == 0.0)
    m = DiversitySimilarity(D)
    m.add_recommendations([3, 7, 1, 9])
    m.add_recommendations([6])
    assert m.get_metric_value() == pytest.approx((got[0, 1] + 0.0) / 2, rel=1e-15) and m.n_evaluated_users == 2
    assert DiversitySimilarity(D).get_metric_value() == 0.0


def test_len_based_denominators():
    counts = np.array([4, 0, 2, 2, 0, 1], dtype=np.int64)
    base = beyond_accuracy_metrics(counts, 1.0, 1.0, 3, 3, 3, 6, 10)
    got = beyond_accuracy_metrics(counts, 1.0, 1.0, 3, 3, 3, 6, 10, ignore_items=np.array([1, 4, 1]), ignore_users=np.array([7, 8]))
    assert got["COVERAGE_ITEM"] == 4 / (6 - 3) and base["COVERAGE_ITEM"] == 4 / 6          # the repeated id counts twice
    assert got["COVERAGE_USER"] == 3 / (10 - 2) and base["COVERAGE_USER"] == 3 / 10
    for k in ("NOVELTY", "AVERAGE_POPULARITY", "DIVERSITY_MEAN_INTER_LIST", "DIVERSITY_GINI", "SHANNON_ENTROPY", "DIVERSITY_HERFINDAHL"):
        assert got[k] == base[k], k                                                        # ignored bins were empty
    cleared = beyond_accuracy_metrics(counts, 1.0, 1.0, 3, 3, 3, 6, 10, ignore_items=np.array([0]))
    rest = beyond_accuracy_metrics(np.array([0, 0, 2, 2, 0, 1]), 1.0, 1.0, 3, 3, 3, 6, 10)
    for k in ("DIVERSITY_GINI", "SHANNON_ENTROPY", "DIVERSITY_HERFINDAHL"):
        assert cleared[k] == rest[k] != base[k], k                                         # a recommended ignored item's bin is cleared
    assert cleared["DIVERSITY_MEAN_INTER_LIST"] == base["DIVERSITY_MEAN_INTER_LIST"]       # MeanInterList does not know the list
    assert cleared["COVERAGE_ITEM"] == 4 / 5


def test_fixture_pins_the_repeated_id(fx):
    assert len(fx["ignore_items"]) == 23 and len(set(fx["ignore_items"].tolist())) == 22
    assert fx["expected"]["holdout_all"]["20"]["COVERAGE_ITEM"] > 1.0      # 159 recommended items over 181 - 23
