"""What the evaluators' one device block loop promises, CPU only: over a recommender that offers the four `evaluate_*_on_device`
hooks, every block goes through the hook in order and the parts add up to the host route's result; one block declined (None) or
out of device memory (MemoryError) sends ALL users down the host route, whose result is then returned exactly.

The recommender is a fake over a fixed random score matrix.  Its hooks form their sums on the host from the public per-user
pieces (RankedListMetrics in float64, rmse_on_test_items, the item weights they are handed), so no GPU is involved.
23 users in blocks of 7: four blocks, the last one ragged."""
import json
import math

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd._lib import EVAL_FULL_METRICS, EVAL_METRICS
from ganmf_amd.evaluation import (FULL_METRICS, EvaluatorHoldoutFast, EvaluatorNegativeItemSampleFast, RankedListMetrics,
                                  rmse_on_test_items)

N_USERS, N_ITEMS, CUTOFFS, BLOCK = 23, 37, [10, 1, 5], 7
BLOCKS = [list(range(lo, min(lo + BLOCK, N_USERS))) for lo in range(0, N_USERS, BLOCK)]
# blocks against one block / block-wise against per-user sums in float64: the bound of tests/test_evaluator_full.py ("fast vs slow")
# and tests/test_negative_sample_evaluator.py (test_fast_blocks_equal_one_block, "blocks vs users")
RTOL = 1e-12


@pytest.fixture(scope="module")
def data():
    rng = np.random.RandomState(11)
    train = (rng.rand(N_USERS, N_ITEMS) < 0.2).astype(np.float32)
    test = ((rng.rand(N_USERS, N_ITEMS) < 0.15) * rng.randint(1, 6, size=(N_USERS, N_ITEMS)) * (train == 0)).astype(np.float32)
    for u in np.flatnonzero(test.sum(axis=1) == 0):                  # every user is evaluated
        test[u, np.flatnonzero(train[u] == 0)[0]] = 3.0
    negative = ((rng.rand(N_USERS, N_ITEMS) < 0.3) * (test == 0)).astype(np.float32)    # some of them seen in training
    return dict(train=sps.csr_matrix(train), test=sps.csr_matrix(test), negative=sps.csr_matrix(negative),
                scores=rng.randn(N_USERS, N_ITEMS).astype(np.float32), groups=rng.randint(-1, 3, size=N_USERS))


class _Fake(object):
    """`fault`: what the hooks do on their third block -- None: nothing, "decline": return None, "oom": raise MemoryError"""

    def __init__(self, data, fault=None, honours=True):
        self.URM_train, self.scores = data["train"], data["scores"]
        self.fault, self.honours_items_to_compute = fault, honours
        self.blocks, self.candidates_given, self.host_users = [], [], []

    def get_URM_train(self):
        return self.URM_train.copy()

    # ---- host methods ------------------------------------------------------------------------------------------------------
    def _rank(self, users, cutoff, remove_seen, items_to_compute):
        scores = self.scores[users].copy()
        if items_to_compute is not None and self.honours_items_to_compute:
            keep = np.zeros(N_ITEMS, dtype=bool)
            keep[items_to_compute] = True
            scores[:, ~keep] = -np.inf
        if remove_seen:
            scores[self.URM_train[users].toarray() != 0] = -np.inf
        lists = []
        for row in scores:
            order = np.argsort(-row, kind="stable")[:cutoff]
            lists.append([int(i) for i in order if np.isfinite(row[i])])
        return lists, scores

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                  remove_CustomItems_flag=False, return_scores=False):
        users = np.atleast_1d(np.asarray(user_id_array))
        self.host_users.extend(int(u) for u in users)
        lists, scores = self._rank(users, cutoff, remove_seen_flag, items_to_compute)
        return (lists, scores) if return_scores else lists

    # ---- device hooks ------------------------------------------------------------------------------------------------------
    def _block(self, users, candidates_csr):
        """records the block; True when the hook is to go on"""
        self.blocks.append([int(u) for u in users])
        self.candidates_given.append(candidates_csr is not None)
        if len(self.blocks) == 3 and self.fault == "oom":
            raise MemoryError("synthetic: out of device memory")
        return not (len(self.blocks) == 3 and self.fault == "decline")

    def _user_rows(self, test, users, cutoffs, remove_seen, candidates_csr, ratings=None, item_weights=None, counts=None):
        """[n, n_cutoffs, 9 or 13] float64: every user's own values (13: + RMSE, novelty, popularity, non-empty)"""
        full = ratings is not None
        out = np.zeros((len(users), len(cutoffs), len(EVAL_FULL_METRICS if full else EVAL_METRICS)))
        for i, u in enumerate(users):
            cand = None
            if candidates_csr is not None:
                cand = candidates_csr.indices[candidates_csr.indptr[u]:candidates_csr.indptr[u + 1]]
            lists, scores = self._rank(np.atleast_1d(u), max(cutoffs), remove_seen, cand)
            t_items, t_ratings = test.indices[test.indptr[u]:test.indptr[u + 1]], test.data[test.indptr[u]:test.indptr[u + 1]]
            scorer = RankedListMetrics(t_items, t_ratings, max(cutoffs), dtype=np.float64)
            hit, gain = scorer.match(np.asarray(lists[0], dtype=np.int64))
            for ci, c in enumerate(cutoffs):
                row = scorer(hit, gain, c)
                out[i, ci, :len(EVAL_METRICS)] = [row[name] for name in EVAL_METRICS]
                if full:
                    listed = np.asarray(lists[0][:c], dtype=np.int64)
                    counts[ci][listed] += 1
                    out[i, ci, len(EVAL_METRICS):] = [rmse_on_test_items(scores[0], t_items, t_ratings), item_weights[0][listed].sum(),
                                                      item_weights[1][listed].sum() / max(len(listed), 1), float(len(listed) > 0)]
        return out

    def evaluate_on_device(self, evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, disc, ideal_cum,
                           remove_seen_flag=True):
        if not self._block(user_id_array, None):
            return None
        return self._user_rows(urm_test_sorted, user_id_array, cutoffs, remove_seen_flag, None).sum(axis=0)

    def evaluate_full_on_device(self, evaluator_key, urm_test_sorted, gains, ratings, item_weights, user_id_array, cutoffs, disc,
                                ideal_cum, remove_seen_flag=True, counts=None):
        if not self._block(user_id_array, None):
            return None
        return self._user_rows(urm_test_sorted, user_id_array, cutoffs, remove_seen_flag, None, ratings, item_weights, counts).sum(axis=0)

    def evaluate_candidates_on_device(self, evaluator_key, urm_test_sorted, gains, candidates_csr, user_id_array, cutoffs, disc,
                                      ideal_cum, remove_seen_flag=True, ratings=None, item_weights=None, counts=None):
        if not self.honours_items_to_compute:
            return None
        if not self._block(user_id_array, candidates_csr):
            return None
        return self._user_rows(urm_test_sorted, user_id_array, cutoffs, remove_seen_flag, candidates_csr, ratings, item_weights,
                               counts).sum(axis=0)

    def evaluate_groups_on_device(self, evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, disc, ideal_cum, group_of,
                                  n_groups, remove_seen_flag=True, candidates_csr=None, per_user=False):
        if candidates_csr is not None and not self.honours_items_to_compute:
            return None
        if not self._block(user_id_array, candidates_csr):
            return None
        rows = self._user_rows(urm_test_sorted, user_id_array, cutoffs, remove_seen_flag, candidates_csr)
        group_of = np.asarray(group_of)
        sums = np.stack([rows[group_of == g].sum(axis=0) for g in range(n_groups)]) if n_groups else np.zeros((0,) + rows.shape[1:])
        sizes = np.array([int((group_of == g).sum()) for g in range(n_groups)], dtype=np.int64)
        return sums, sizes, rows if per_user else None


def _evaluator(data, route, full=False):
    if route == "candidates":
        ev = EvaluatorNegativeItemSampleFast(data["test"], data["negative"], CUTOFFS, full_metrics=full)
    else:
        ev = EvaluatorHoldoutFast(data["test"], CUTOFFS, full_metrics=full)
    ev._block_size = BLOCK
    assert ev._users.tolist() == list(range(N_USERS))
    return ev


def _host(data, route, full=False, by_group=False, honours=True):
    """(the host route's result, the users its host methods were asked for)"""
    ev, rec = _evaluator(data, route, full), _Fake(data, honours=honours)
    ev.use_device_metrics = False
    got = ev.evaluateRecommenderByGroup(rec, data["groups"], return_per_user=True) if by_group else ev.evaluateRecommender(rec)[0]
    assert rec.blocks == []
    return got, rec.host_users


def _close(got, want, what):
    if math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= 1e-15 + RTOL * abs(want), (what, got, want)


def _close_rows(got, want, keys):
    assert list(got) == list(want) == CUTOFFS
    for c in CUTOFFS:
        assert list(got[c]) == list(want[c]) and set(got[c]) == set(keys), c     # the host route's keys, in its order
        for k in keys:
            _close(got[c][k], want[c][k], (c, k))


ROWS = [("full_width", False), ("full_width", True), ("candidates", False), ("candidates", True)]


@pytest.mark.parametrize("route,full", ROWS)
def test_every_block_accepted_adds_up_to_the_host_result(data, route, full):
    rec = _Fake(data)
    got, text = _evaluator(data, route, full).evaluateRecommender(rec)
    assert rec.blocks == BLOCKS and rec.host_users == []                 # four calls, the blocks in order, nothing on the host
    assert rec.candidates_given == [route == "candidates"] * 4
    want, _ = _host(data, route, full)
    _close_rows(got, want, FULL_METRICS if full else FULL_METRICS[:11])
    assert all(np.isfinite(got[c]["RMSE"]) if full else math.isnan(got[c]["RMSE"]) for c in CUTOFFS)
    assert "CUTOFF: 10 - ROC_AUC: " in text


@pytest.mark.parametrize("fault", ["decline", "oom"])
@pytest.mark.parametrize("route,full", ROWS)
def test_a_refused_third_block_sends_every_user_to_the_host_route(data, route, full, fault):
    rec = _Fake(data, fault=fault)
    got, _ = _evaluator(data, route, full).evaluateRecommender(rec)
    assert rec.blocks == BLOCKS[:3]                                      # no block after the refused one
    want, host_users = _host(data, route, full)
    assert json.dumps(got) == json.dumps(want)                           # == on every value (NaN RMSE of the nine-metric rows included)
    assert rec.host_users == host_users and sorted(set(host_users)) == list(range(N_USERS))


def _same_groups(got, want, exact):
    (res, users, ids), (w_res, w_users, w_ids) = got, want
    assert ids.tolist() == w_ids.tolist() == list(range(N_USERS))
    if exact:
        assert json.dumps(res) == json.dumps(w_res) and np.array_equal(users, w_users)
        return
    np.testing.assert_allclose(users, w_users, rtol=RTOL, atol=1e-15)
    assert list(res) == list(w_res) == [0, 1, 2]
    for g in res:
        assert res[g]["n_users"] == w_res[g]["n_users"] > 0
        _close_rows({c: res[g][c] for c in CUTOFFS}, {c: w_res[g][c] for c in CUTOFFS}, EVAL_METRICS + ("F1",))


@pytest.mark.parametrize("per_user", [False, True])
@pytest.mark.parametrize("route", ["full_width", "candidates"])
def test_groups_every_block_accepted(data, route, per_user):
    rec = _Fake(data)
    got = _evaluator(data, route).evaluateRecommenderByGroup(rec, data["groups"], return_per_user=per_user)
    assert rec.blocks == BLOCKS and rec.host_users == [] and rec.candidates_given == [route == "candidates"] * 4
    want, _ = _host(data, route, by_group=True)
    if per_user:
        _same_groups(got, want, exact=False)
    else:
        _same_groups((got, want[1], want[2]), want, exact=False)


@pytest.mark.parametrize("fault", ["decline", "oom"])
@pytest.mark.parametrize("per_user", [False, True])
@pytest.mark.parametrize("route", ["full_width", "candidates"])
def test_groups_a_refused_third_block_sends_every_user_to_the_host_route(data, route, per_user, fault):
    rec = _Fake(data, fault=fault)
    got = _evaluator(data, route).evaluateRecommenderByGroup(rec, data["groups"], return_per_user=per_user)
    assert rec.blocks == BLOCKS[:3]
    want, host_users = _host(data, route, by_group=True)
    _same_groups(got if per_user else (got, want[1], want[2]), want, exact=True)
    assert rec.host_users == host_users and sorted(set(host_users)) == list(range(N_USERS))


@pytest.mark.parametrize("full", [False, True])
def test_recommender_that_ignores_items_to_compute_takes_the_full_width_routes(data, full):
    """honours_items_to_compute = False: the candidate hooks decline, and the negative-sample class goes down the full-width
    routes -- device first, every block through the full-width hook -- exactly as EvaluatorHoldoutFast does"""
    rec = _Fake(data, honours=False)
    got, _ = _evaluator(data, "candidates", full).evaluateRecommender(rec)
    assert rec.blocks == BLOCKS and rec.candidates_given == [False] * 4 and rec.host_users == []
    plain = _Fake(data, honours=False)
    want, _ = _evaluator(data, "full_width", full).evaluateRecommender(plain)
    assert json.dumps(got) == json.dumps(want) and plain.blocks == BLOCKS
    if not full:
        rec = _Fake(data, honours=False)
        grouped = _evaluator(data, "candidates").evaluateRecommenderByGroup(rec, data["groups"], return_per_user=True)
        assert rec.blocks == BLOCKS and rec.candidates_given == [False] * 4 and rec.host_users == []
        want = _evaluator(data, "full_width").evaluateRecommenderByGroup(_Fake(data, honours=False), data["groups"], return_per_user=True)
        _same_groups(grouped, want, exact=True)
        # and with the device route closed, the full-width host route
        host, _ = _host(data, "candidates", honours=False)
        assert json.dumps(host) == json.dumps(_host(data, "full_width", honours=False)[0])
