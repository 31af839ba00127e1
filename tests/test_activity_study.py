"""The user-activity study's bucket rule (ganmf_amd/studies.py) and the host routes of evaluateRecommenderByGroup (CPU only),
against the stored per-user AP of the reference's own recommend + average_precision (tools/make_activity_study_golden.py):
users in every bucket, a count exactly on a bound, graded ratings, a short list, a user without a hit, users without a test item.

Tolerance 1e-12 * max(1, |v|): the per-user values are float64 on both sides and differ only in the order of a handful of
additions and in j * (1 / rank) against j / rank (the figure tests/test_gpu_recommend.py holds the device to against the host)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd._lib import EVAL_METRICS
from ganmf_amd.base import BaseRecommender
from ganmf_amd.evaluation import (EvaluatorHoldout, EvaluatorHoldoutFast, EvaluatorNegativeItemSample,
                                  EvaluatorNegativeItemSampleFast)
from ganmf_amd.studies import activity_bucket, activity_bucket_keys

MAP = EVAL_METRICS.index("MAP")


def _close(got, want, what):
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (what, got, want)


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


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "activity_study_expected.json")))
    for key in ("train", "test", "negative"):
        g[key] = sps.csr_matrix(np.array(g[key], np.float32))
    g["U"], g["V"] = np.array(g["U"], np.float32), np.array(g["V"], np.float32)
    return g


def _groups(g):
    """the study's buckets as user groups, user 3 taken out (-1)"""
    counts = np.asarray((g["train"] + g["test"]).sum(axis=1)).reshape(-1)
    groups = activity_bucket(counts, g["bounds"])
    groups[3] = -1
    return groups


def test_bucket_keys_and_the_key_the_reference_figure_drops():
    keys, plotted = activity_bucket_keys([25, 100, 500, 1000])                 # MFLearned.py:73, the MovieLens bounds
    assert keys == ["<25", ">=25, <100", ">=100, <500", ">=500, <1000", ">=1000"]
    assert plotted == [True, True, True, False, True]                          # build_xticks lists four of the five
    keys, plotted = activity_bucket_keys([10, 20])
    assert keys == ["<10", ">=10, <20", ">=20"] and plotted == [True, False, True]
    keys, plotted = activity_bucket_keys([7])                                  # a single bound: the x-ticks hold only '<7'
    assert keys == ["<7", ">=7"] and plotted == [True, False]
    with pytest.raises(ValueError):
        activity_bucket_keys([])


def test_bucket_of_a_count_by_hand():
    bounds = [25, 100, 500, 1000]
    keys, _ = activity_bucket_keys(bounds)
    table = {0: "<25", 24: "<25", 24.5: "<25", 25: ">=25, <100", 99: ">=25, <100", 100: ">=100, <500", 499.5: ">=100, <500",
             500: ">=500, <1000", 999: ">=500, <1000", 1000: ">=1000", 123456: ">=1000"}
    got = activity_bucket(np.array(list(table), dtype=np.float64), bounds)
    assert [keys[b] for b in got] == list(table.values())
    for i, b in enumerate(bounds):                                             # exactly on a bound: the bucket that starts there
        assert keys[activity_bucket([b], bounds)[0]].startswith(">=%d" % b) and activity_bucket([b], bounds)[0] == i + 1


def test_golden_case_is_the_one_described(golden):
    g = golden
    counts = np.asarray((g["train"] + g["test"]).sum(axis=1)).reshape(-1)
    nnz = np.ediff1d(g["train"].indptr) + np.ediff1d(g["test"].indptr)
    bucket = activity_bucket(counts, g["bounds"])
    who = g["users"]
    with_test = np.ediff1d(g["test"].indptr) > 0
    assert set(bucket[with_test]) == set(range(len(g["bounds"]) + 1))          # every bucket, the dropped one included
    assert counts[who["on_bound"]] == g["bounds"][1] and bucket[who["on_bound"]] == 2
    assert np.any(counts != nnz)                                               # value sum, not nnz
    assert all(g["ap"]["20"][u] is None and not with_test[u] for u in who["no_test"])
    assert g["ap"]["20"][who["no_hit"]] == 0.0
    assert g["test"].shape[1] - g["train"][who["short_list"]].nnz < 20


@pytest.mark.parametrize("cls", [EvaluatorHoldout, EvaluatorHoldoutFast])
def test_holdout_per_user_map_matches_the_reference(golden, cls):
    g = golden
    ev = cls(g["test"], g["cutoffs"])
    res, per_user, users = ev.evaluateRecommenderByGroup(_Factors(g["train"], g["U"], g["V"]), _groups(g), return_per_user=True)
    assert per_user.shape == (len(users), len(g["cutoffs"]), 9) and users.tolist() == list(ev.usersToEvaluate)
    assert set(users.tolist()) == {u for u, v in enumerate(g["ap"]["20"]) if v is not None}
    for ci, c in enumerate(g["cutoffs"]):
        for i, u in enumerate(users):
            _close(per_user[i, ci, MAP], g["ap"][str(c)][u], (cls.__name__, c, u))
    assert set(res) == set(range(len(g["bounds"]) + 1))


@pytest.mark.parametrize("cls", [EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast])
def test_negative_sample_per_user_map_matches_the_reference(golden, cls):
    g = golden
    ev = cls(g["test"], g["negative"], g["cutoffs"])
    _, per_user, users = ev.evaluateRecommenderByGroup(_Factors(g["train"], g["U"], g["V"]), _groups(g), return_per_user=True)
    differs = 0
    for ci, c in enumerate(g["cutoffs"]):
        for i, u in enumerate(users):
            _close(per_user[i, ci, MAP], g["ap_candidates"][str(c)][u], (cls.__name__, c, u))
            differs += g["ap_candidates"][str(c)][u] != g["ap"][str(c)][u]
    assert differs > 10                                                        # the candidate ranking is another ranking


def _fast(cls, g, **kw):
    ev = cls(g["test"], g["negative"], g["cutoffs"], **kw) if cls is EvaluatorNegativeItemSampleFast else cls(g["test"], g["cutoffs"], **kw)
    ev.use_device_metrics = False
    return ev


@pytest.mark.parametrize("cls", [EvaluatorHoldoutFast, EvaluatorNegativeItemSampleFast])
@pytest.mark.parametrize("min_ratings", [1, 3])
def test_weighted_group_means_are_the_means_over_the_same_users(golden, cls, min_ratings):
    """every user with a test item in some group: the group means weighted by n_users are evaluateRecommender's means (the Fast
    classes' float64 host route), every metric and cut-off, F1 from those means"""
    g = golden
    rec = _Factors(g["train"], g["U"], g["V"])
    counts = np.asarray((g["train"] + g["test"]).sum(axis=1)).reshape(-1)
    ev = _fast(cls, g, minRatingsPerUser=min_ratings)
    res = ev.evaluateRecommenderByGroup(rec, activity_bucket(counts, g["bounds"]))
    whole, _ = ev.evaluateRecommender(rec)
    n = sum(r["n_users"] for r in res.values())
    assert n == len(ev.usersToEvaluate) > 0
    for c in g["cutoffs"]:
        for name in EVAL_METRICS:
            _close(sum(r["n_users"] * r[c][name] for r in res.values()) / n, whole[c][name], (cls.__name__, c, name))
        p = sum(r["n_users"] * r[c]["PRECISION"] for r in res.values()) / n
        rc = sum(r["n_users"] * r[c]["RECALL"] for r in res.values()) / n
        _close(2 * p * rc / (p + rc), whole[c]["F1"], (cls.__name__, c, "F1"))
        for r in res.values():
            assert set(r[c]) == set(EVAL_METRICS) | {"F1"}
            if r["n_users"]:
                pg, rg = r[c]["PRECISION"], r[c]["RECALL"]
                _close(r[c]["F1"], 2 * pg * rg / (pg + rg) if pg + rg else 0.0, (cls.__name__, c, "group F1"))


@pytest.mark.parametrize("cls", [EvaluatorHoldout, EvaluatorHoldoutFast, EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast])
def test_reference_order_and_fast_classes_agree(golden, cls):
    """all four classes form the grouped row from the same float64 per-user values"""
    g = golden
    rec = _Factors(g["train"], g["U"], g["V"])
    neg = cls in (EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast)
    ev = cls(g["test"], g["negative"], g["cutoffs"]) if neg else cls(g["test"], g["cutoffs"])
    ref = _fast(EvaluatorNegativeItemSampleFast if neg else EvaluatorHoldoutFast, g)
    got, want = ev.evaluateRecommenderByGroup(rec, _groups(g)), ref.evaluateRecommenderByGroup(rec, _groups(g))
    assert json.dumps(got) == json.dumps(want)


@pytest.mark.parametrize("cls", [EvaluatorHoldout, EvaluatorHoldoutFast])
def test_users_outside_the_groups_are_in_no_group(golden, cls):
    g = golden
    rec = _Factors(g["train"], g["U"], g["V"])
    n_users = g["test"].shape[0]
    n_test = np.ediff1d(g["test"].indptr)
    groups = np.arange(n_users) % 2
    groups[[3, 4, 8]] = -1
    groups[9] = 7                                                              # a group of one; group values need not be dense
    ev = cls(g["test"], g["cutoffs"], minRatingsPerUser=3)
    res, per_user, users = ev.evaluateRecommenderByGroup(rec, groups, return_per_user=True)
    assert sorted(res) == [0, 1, 7] and res[7]["n_users"] == 1
    assert users.tolist() == np.flatnonzero(n_test >= 3).tolist()              # -1 users are evaluated, users below the minimum are not
    for label in (0, 1, 7):
        members = [i for i, u in enumerate(users) if groups[u] == label]
        assert res[label]["n_users"] == len(members) and not set(users[members]) & {0, 1, 3, 4, 8}
        for ci, c in enumerate(g["cutoffs"]):
            for mi, name in enumerate(EVAL_METRICS):
                _close(res[label][c][name], per_user[members, ci, mi].sum() / len(members), (label, c, name))
    only = np.full(n_users, -1)
    only[0] = 5                                                                # its only member has no test item: an empty group
    res = ev.evaluateRecommenderByGroup(rec, only)
    assert res == {5: dict({c: dict.fromkeys(EVAL_METRICS + ("F1",), 0.0) for c in g["cutoffs"]}, n_users=0)}
    with pytest.raises(ValueError):
        ev.evaluateRecommenderByGroup(rec, np.full(n_users, -2))
    with pytest.raises(ValueError):
        ev.evaluateRecommenderByGroup(rec, np.zeros(n_users - 1, dtype=np.int64))
