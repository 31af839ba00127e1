"""Candidate scoring and top-k on the device (ganmf_amd/csrc/cand_topk.hpp) through the C ABI -- ganmf_set_candidates_csr,
ganmf_recommend_candidates, ganmf_evaluate_candidates -- and through EvaluatorNegativeItemSampleFast.

Exact comparisons use factors on the grid {-1, -3/4, ..., 1} with k <= 600: every product is a multiple of 1/16 and every sum
stays below 2^10, so a dot product is exact in fp32 in any order (and through the split-bf16 scoring GEMM), and ids and scores
can be compared bit for bit with a ranking formed here in float64."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from test_gpu_gemm import _mk

pytestmark = pytest.mark.gpu

_SUM_BASED = {"ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "F1", "HIT_RATE", "ARHR"}


def _grid(rng, shape):
    return (rng.randint(-4, 5, size=shape) / 4.0).astype(np.float32)


def _engine(U, V):
    from ganmf_amd.engine import Engine
    eng = Engine(U.shape[0], V.shape[0], U.shape[1], 16, 32)
    eng.set_tensor(100, U)
    eng.set_tensor(101, V)
    return eng


def _csr(rows, n_cols, rng=None, messy=False):
    """CSR whose row r stores the ids rows[r]; messy: shuffled inside the row and with one id repeated"""
    indptr, indices = [0], []
    for items in rows:
        items = np.asarray(items, dtype=np.int64)
        if messy and len(items):
            items = np.concatenate([rng.permutation(items), items[:1]])
        indices.append(items)
        indptr.append(indptr[-1] + len(items))
    indices = np.concatenate(indices) if indices else np.zeros(0, np.int64)
    return sps.csr_matrix((np.ones(len(indices), np.float32), indices.astype(np.int32), np.asarray(indptr, np.int64)),
                          shape=(len(rows), n_cols))


def _ranked(scores_row, cand, masked):
    """(ids, scores) of one row's candidates in the order the kernel must return them: score descending, ties to the smaller
    id (np.lexsort((item, -score))), masked candidates dropped"""
    cand = np.asarray(cand, dtype=np.int64)
    s = scores_row[cand].astype(np.float64)
    s[np.isin(cand, masked)] = -np.inf
    order = np.lexsort((cand, -s))
    order = order[np.isfinite(s[order])]
    return cand[order], s[order]


def _expect(ranked, ids, cutoff):
    items = np.full((len(ids), cutoff), -1, dtype=np.int32)
    vals = np.full((len(ids), cutoff), -np.inf, dtype=np.float32)
    for i, r in enumerate(ids):
        it, s = ranked[r]
        n = min(len(it), cutoff)
        items[i, :n], vals[i, :n] = it[:n], s[:n]
    return items, vals


def _lists(rng, n_rows, width, counts):
    """row r holds counts[r % len(counts)] random distinct ids, ascending"""
    return [np.sort(rng.choice(width, size=min(counts[r % len(counts)], width), replace=False)) for r in range(n_rows)]


def _seen_lists(rng, cands, width):
    """every third candidate of the row (seen and candidate) plus five ids drawn from everything"""
    return [np.unique(np.concatenate([c[::3], rng.choice(width, size=5, replace=False)])) for c in cands]


@pytest.mark.parametrize("k", [1, 3, 64, 65, 250, 257, 600])
def test_ranking_ties_and_structural_edges_user_mode(k):
    """k around the 64-float row padding and the one- / two-register-pass boundary (ld 64, 128, 256, 320), and k = 600 (ld 640 >
    512: the row's factor in LDS behind the candidate slots, with the longest list more than 64 KiB of dynamic LDS; sums of 600
    multiples of 1/16 stay below 2^10, still exact in fp32); lists of 0, 1,
    cutoff - 1, cutoff, 255 / 256 / 257 (the 256-thread scan) and GANMF_CANDIDATES_MAX_PER_ROW candidates; n = 1 and 257 (two
    metric blocks' worth of rows), ids unsorted and repeated; candidate rows uploaded shuffled and with a repeat"""
    from ganmf_amd._lib import CANDIDATES_MAX_PER_ROW as CMAX
    rng = np.random.RandomState(100 + k)
    nu, ni = 40, CMAX + 8
    U, V = _grid(rng, (nu, k)), _grid(rng, (ni, k))
    scores = U.astype(np.float64) @ V.astype(np.float64).T
    cands = _lists(rng, nu, ni, [0, 1, 4, 5, 255, 256, 257, CMAX, 100, 300])
    seen = _seen_lists(rng, cands, ni)
    eng = _engine(U, V)
    eng.set_candidates(_csr(cands, ni, rng, messy=True))
    eng.set_seen(_csr(seen, ni))
    many = rng.randint(0, nu, size=257)
    many[:10] = np.arange(10)[::-1]                                     # every list length is asked for, in descending row order
    ties = 0
    for remove_seen in (False, True):
        ranked = [_ranked(scores[r], cands[r], seen[r] if remove_seen else []) for r in range(nu)]
        ties += sum(int((np.diff(s) == 0).sum()) for _, s in ranked)
        for cutoff in (1, 5, 256):
            for ids in (np.array([7]), many):
                items, vals = eng.recommend_candidates(ids, cutoff, remove_seen=remove_seen)
                want_items, want_vals = _expect(ranked, ids, cutoff)
                np.testing.assert_array_equal(items, want_items)
                np.testing.assert_array_equal(vals, want_vals)
    assert ties > 100                                                   # the tie rule was exercised
    eng.close()


def test_ranking_item_mode():
    """transposed = 1: the requested rows are rows of V, the candidates rows of U"""
    rng = np.random.RandomState(7)
    k, n_gen_users, n_gen_items = 65, 300, 270       # evaluation orientation: 270 users x 300 items
    U, V = _grid(rng, (n_gen_users, k)), _grid(rng, (n_gen_items, k))
    scores = V.astype(np.float64) @ U.astype(np.float64).T
    cands = _lists(rng, n_gen_items, n_gen_users, [0, 1, 4, 5, 255, 256, 257, 300])
    seen = _seen_lists(rng, cands, n_gen_users)
    eng = _engine(U, V)
    eng.set_candidates(_csr(cands, n_gen_users, rng, messy=True))
    eng.set_seen(_csr(seen, n_gen_users))
    ids = rng.randint(0, n_gen_items, size=257)
    for remove_seen in (False, True):
        ranked = [_ranked(scores[r], cands[r], seen[r] if remove_seen else []) for r in range(n_gen_items)]
        for cutoff in (1, 5, 256):
            items, vals = eng.recommend_candidates(ids, cutoff, transposed=True, remove_seen=remove_seen)
            want_items, want_vals = _expect(ranked, ids, cutoff)
            np.testing.assert_array_equal(items, want_items)
            np.testing.assert_array_equal(vals, want_vals)
    eng.close()


def test_score_filter_item_mask_and_cold_row():
    rng = np.random.RandomState(3)
    nu, ni, k = 30, 90, 3
    U, V = _grid(rng, (nu, k)), _grid(rng, (ni, k))
    scores = U.astype(np.float64) @ V.astype(np.float64).T
    cands = _lists(rng, nu, ni, [40, 7, 90])
    seen = _seen_lists(rng, cands, ni)
    seen[4] = np.zeros(0, np.int64)                                       # row 4 has no training interaction: cold
    allowed = np.sort(rng.choice(ni, size=30, replace=False))
    eng = _engine(U, V)
    eng.set_candidates(_csr(cands, ni))
    eng.set_seen(_csr(seen, ni))
    eng.set_score_filter(allowed, mask_cold=True)
    ids = np.arange(nu)
    outside = np.setdiff1d(np.arange(ni), allowed)
    for remove_seen in (False, True):
        ranked = [_ranked(scores[r], cands[r], np.concatenate([outside, seen[r] if remove_seen else []])) for r in range(nu)]
        ranked[4] = (np.zeros(0, np.int64), np.zeros(0))
        items, vals = eng.recommend_candidates(ids, 10, remove_seen=remove_seen)
        want_items, want_vals = _expect(ranked, ids, 10)
        np.testing.assert_array_equal(items, want_items)
        np.testing.assert_array_equal(vals, want_vals)
        assert np.all(items[4] == -1) and np.all(np.isin(items[items >= 0], allowed))
    eng.set_score_filter(None, mask_cold=False)                            # and without the filter the cold row is ranked again
    items, _ = eng.recommend_candidates(ids, 10, remove_seen=False)
    np.testing.assert_array_equal(items, _expect([_ranked(scores[r], cands[r], []) for r in range(nu)], ids, 10)[0])
    eng.close()


def test_scores_on_generic_factors_within_the_fp32_gemm_bound():
    """random fp32 factors, k = 250: every candidate's score against the float64 product, within the bound tests/test_gpu_gemm.py
    holds the fp32 GEMM to (4e-7 * sum|a||b| * sqrt(K)); the candidate dot product is an fp32 FMA chain of at most 4 terms per
    lane and a 64-way tree, well inside it"""
    rng = np.random.RandomState(11)
    nu, ni, k = 70, 500, 250
    U, V, ref, bound = _mk(rng, nu, ni, k, False, False)
    cands = _lists(rng, nu, ni, [100, 256, 33])
    eng = _engine(U, V)
    eng.set_candidates(_csr(cands, ni))
    ids = np.arange(nu)
    items, vals = eng.recommend_candidates(ids, 256, remove_seen=False)
    for r in ids:
        n = len(cands[r])
        got = items[r, :n].astype(np.int64)
        assert np.all(items[r, n:] == -1) and sorted(got.tolist()) == cands[r].tolist()
        assert np.all(np.diff(vals[r, :n]) <= 0)
        err = np.abs(vals[r, :n].astype(np.float64) - ref[r, got])
        assert np.all(err <= 4e-7 * bound[r, got] * np.sqrt(k) + 1e-30), float((err / bound[r, got]).max())
    eng.close()


def _eval_inputs(rng, nu, ni, cutoffs):
    """test matrix (graded, sorted rows), gains, ratings, disc / ideal_cum and item weights as the evaluators form them"""
    from ganmf_amd.evaluation import EvaluatorHoldoutFast, popularity_weights
    t = ((rng.rand(nu, ni) < 0.05) * rng.randint(1, 6, size=(nu, ni))).astype(np.float32)
    t[np.arange(nu), rng.randint(0, ni, nu)] = 3.0
    ev = EvaluatorHoldoutFast(sps.csr_matrix(t), cutoffs)
    weights = popularity_weights(rng.randint(0, 50, size=ni) + 1)
    return ev, weights


@pytest.mark.parametrize("mode", ["user", "item"])
def test_whole_catalogue_candidates_equal_full_width_evaluation(mode):
    """every row's candidates = all W = 300 items: ganmf_evaluate_candidates must return the bits of ganmf_evaluate and of
    ganmf_evaluate_full (sums; counts as integers) on grid factors, 300 rows = two metric blocks"""
    rng = np.random.RandomState(21)
    transposed = mode == "item"
    n_rows, W, k = 300, 300, 17
    rows_f, cols_f = _grid(rng, (n_rows, k)), _grid(rng, (W, k))
    eng = _engine(cols_f, rows_f) if transposed else _engine(rows_f, cols_f)
    cutoffs = [1, 5, 20]
    ev, weights = _eval_inputs(rng, n_rows, W, cutoffs)
    seen = sps.csr_matrix((rng.rand(n_rows, W) < 0.1).astype(np.float32))
    eng.set_seen(seen)
    eng.set_candidates(sps.csr_matrix(np.ones((n_rows, W), np.float32)))
    eng.set_test(ev._test_sorted, ev._test_gain)
    eng.set_test_ratings(ev._test_rating)
    eng.set_eval_item_weights(*weights)
    ids = rng.permutation(n_rows)
    ideal = ev._ideal_cum[ids]
    for remove_seen in (True, False):
        kw = dict(transposed=transposed, remove_seen=remove_seen)
        want = eng.evaluate(ids, cutoffs, ev._disc, ideal, **kw)
        got = eng.evaluate_candidates(ids, cutoffs, ev._disc, ideal, **kw)
        assert got.shape == (3, 9) and got.tobytes() == want.tobytes()
        want_sums, want_counts = eng.evaluate_full(ids, cutoffs, ev._disc, ideal, **kw)
        got_sums, got_counts = eng.evaluate_candidates(ids, cutoffs, ev._disc, ideal, full=True, **kw)
        assert got_sums.shape == (3, 13) and got_sums.tobytes() == want_sums.tobytes()
        assert np.isfinite(got_sums[:, 9]).all()
        np.testing.assert_array_equal(got_counts, want_counts)
        assert got_counts.sum() == len(ids) * sum(cutoffs)
    eng.close()


@pytest.mark.parametrize("mode", ["user", "item"])
def test_rmse_over_candidate_subsets_against_float64(mode):
    """cand_topk_rmse_kernel on proper candidate subsets (candidate position != item id): the RMSE sum of
    ganmf_evaluate_candidates against per-row values formed here in float64.  Per row: test items that are candidates and not
    seen count, a seen candidate (-inf) and a test item outside the candidates (-inf under the items_to_compute rule) drop out.
    Grid factors with k = 17: every error d is a multiple of 1/16 below 2^5, d * d exact in fp32, the device's float64 sum exact,
    so a row's value is the float64 one rounded to fp32 once (the double root adds 2^-53): the sum over the rows is held to
    2^-23 relative."""
    rng = np.random.RandomState(61)
    transposed = mode == "item"
    n_rows, W, k = 300, 200, 17
    rows_f, cols_f = _grid(rng, (n_rows, k)), _grid(rng, (W, k))
    scores = rows_f.astype(np.float64) @ cols_f.astype(np.float64).T
    eng = _engine(cols_f, rows_f) if transposed else _engine(rows_f, cols_f)
    cands = _lists(rng, n_rows, W, [40, 3, 120, 64, 65])
    seen = _seen_lists(rng, cands, W)
    t = np.zeros((n_rows, W), np.float32)
    want = np.zeros(n_rows)
    for r in range(n_rows):
        free = np.setdiff1d(cands[r], seen[r])                          # at least one unseen candidate is a test item
        inside = np.concatenate([free[:2], np.intersect1d(cands[r], seen[r])[:1]])
        outside = np.setdiff1d(np.arange(W), cands[r])[:2]
        t[r, np.concatenate([inside, outside])] = rng.randint(1, 6, size=len(inside) + len(outside))
        d = scores[r, free[:2]] - t[r, free[:2]]
        want[r] = np.sqrt(np.sum(d * d) / len(d))
    from ganmf_amd.evaluation import EvaluatorHoldoutFast, popularity_weights
    cutoffs = [1, 5]
    ev = EvaluatorHoldoutFast(sps.csr_matrix(t), cutoffs)
    eng.set_seen(_csr(seen, W))
    eng.set_candidates(_csr(cands, W, rng, messy=True))
    eng.set_test(ev._test_sorted, ev._test_gain)
    eng.set_test_ratings(ev._test_rating)
    eng.set_eval_item_weights(*popularity_weights(rng.randint(0, 50, size=W) + 1))
    ids = rng.permutation(n_rows)
    sums, _ = eng.evaluate_candidates(ids, cutoffs, ev._disc, ev._ideal_cum[ids], transposed=transposed, remove_seen=True, full=True)
    assert np.all(np.isfinite(sums[:, 9])) and want.min() > 0
    for ci in range(len(cutoffs)):
        assert abs(sums[ci, 9] - want.sum()) <= 2.0 ** -23 * want.sum(), (sums[ci, 9], want.sum())
    # without the seen mask the seen candidate's error counts too
    sums, _ = eng.evaluate_candidates(ids, cutoffs, ev._disc, ev._ideal_cum[ids], transposed=transposed, remove_seen=False, full=True)
    want_all = np.zeros(n_rows)
    for r in range(n_rows):
        inside = np.intersect1d(np.flatnonzero(t[r]), cands[r])
        d = scores[r, inside] - t[r, inside]
        want_all[r] = np.sqrt(np.sum(d * d) / len(d))
    assert abs(sums[0, 9] - want_all.sum()) <= 2.0 ** -23 * want_all.sum(), (sums[0, 9], want_all.sum())
    assert abs(want_all.sum() - want.sum()) > 1e-3 * want.sum()
    eng.close()


def _distinct_exact_model(mode, contract, rng, n_users=300, n_items=60):
    """GANMF with exact AND pairwise distinct scores per user: grid factors in coordinates 1.., and coordinate 0 adds i / 1024 to
    item i's score (below the grid's 1/16 step for i < 64), so no ranking anywhere depends on a tie rule or on rounding"""
    from ganmf_amd.GANMF import GANMF
    assert n_items <= 64
    k = 6
    m = (rng.rand(n_users, n_items) < 0.3).astype(np.float32)
    m[np.arange(n_users), rng.randint(0, n_items, n_users)] = 1.0
    m[5, :] = 0.0                                                     # a cold user (empty list under "mf")
    urm = sps.csr_matrix(m)
    P, Q = _grid(rng, (n_users, k)), _grid(rng, (n_items, k))         # evaluation users / items
    P[:, 0] = 1.0
    Q[:, 0] = np.arange(n_items) / 1024.0
    model = GANMF(urm, mode=mode, is_experiment=True, score_contract=contract)
    model._build(k, 16, 32)
    model.engine.set_tensor(100, Q if mode == "item" else P)
    model.engine.set_tensor(101, P if mode == "item" else Q)
    model.URM_train = model._URM_eval
    return model, m


def _counted(model, name, fn):
    """fn() with every call of model.<name> counted and required to take the device route (not None)"""
    n = [0]
    orig = getattr(model, name)

    def wrapper(*a, **k):
        n[0] += 1
        out = orig(*a, **k)
        assert out is not None
        return out
    setattr(model, name, wrapper)
    try:
        return fn(), n[0]
    finally:
        delattr(model, name)


@pytest.mark.parametrize("mode", ["user", "item"])
@pytest.mark.parametrize("full", [False, True])
def test_fast_class_device_route_equals_its_host_route(mode, full):
    """1e-12 on every sum-based value, the figure of test_device_metrics_equal_host_metrics.
    RMSE (full row) cannot meet 1e-12: a user's RMSE is an fp32 value on both routes (the kernel stores the row's fp32 RMSE, the
    host route gets numpy's float32 one), and only the sum over the users is float64.  With the exact scores of this model the
    fp32 errors d and d*d are the same bits on both sides; the device adds the n squares in float64 (exact) and rounds once
    (2^-24), numpy adds them in float32 (<= n * 2^-24 on the sum, half of it after the root) and rounds the division and the
    root (2 * 2^-24).  With n <= 16 test items per user (asserted) the per-user values, and so their mean, differ by at most
    (16 / 2 + 3) * 2^-24 = 6.6e-7: the bound is 1e-6.  Every evaluated user keeps an unseen test item and none is cold, so the
    RMSE of every row is finite and the comparison is one of numbers."""
    from ganmf_amd.evaluation import FULL_METRICS, EvaluatorNegativeItemSampleFast
    rng = np.random.RandomState(31)
    model, m = _distinct_exact_model(mode, "mf", rng)
    nu, ni = m.shape
    t = ((rng.rand(nu, ni) < 0.08) * rng.randint(1, 6, size=(nu, ni))).astype(np.float32)
    t[rng.rand(nu) < 0.1] = 0
    neg = (rng.rand(nu, ni) < 0.3).astype(np.float32)
    t[7, np.flatnonzero(m[7])[0]] = 4.0                               # a seen test item
    t[5, :] = 0                                                       # the cold user is not evaluated (its RMSE would be NaN)
    for u in np.flatnonzero(t.sum(axis=1)):                           # every evaluated user keeps an unseen test item
        t[u, np.flatnonzero(m[u] == 0)[0]] = 3.0
    assert (t != 0).sum(axis=1).max() <= 16
    cut = [1, 5, 10, 20]
    ev = EvaluatorNegativeItemSampleFast(sps.csr_matrix(t), sps.csr_matrix(neg), cut, full_metrics=full)
    (dev, _), calls = _counted(model, "evaluate_candidates_on_device", lambda: ev.evaluateRecommender(model))
    assert calls == 1
    ev._block_size = 37
    (blocks, _), calls = _counted(model, "evaluate_candidates_on_device", lambda: ev.evaluateRecommender(model))
    assert calls == -(-len(ev._users) // 37)
    ev._block_size = None
    ev.use_device_metrics = False
    host, _ = ev.evaluateRecommender(model)
    for c in cut:
        assert list(dev[c]) == list(host[c]) and (not full or list(dev[c]) == list(FULL_METRICS))
        for name, v in host[c].items():
            for got in (dev[c][name], blocks[c][name]):
                if math.isnan(v):
                    assert math.isnan(got), (c, name)
                else:
                    tol = 1e-6 if name == "RMSE" else 1e-12
                    assert abs(got - v) <= tol * max(1.0, abs(v)), (mode, full, c, name, got, v)
    assert host[5]["MAP"] > 0 and host[20]["NDCG"] > 0
    if full:
        assert all(np.isfinite(r[c]["RMSE"]) and r[c]["RMSE"] > 0 for r in (dev, blocks, host) for c in cut)
    model.engine.close()


def _golden(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "negative_sample_expected.json")))
    for key in ("train", "test", "negative"):
        g[key] = sps.csr_matrix(np.array(g[key], np.float32))
    g["U"], g["V"] = np.array(g["U"], np.float32), np.array(g["V"], np.float32)
    return g


def _golden_model(g, contract):
    from ganmf_amd.GANMF import GANMF
    model = GANMF(g["train"], mode="user", is_experiment=True, score_contract=contract)
    model._build(g["U"].shape[1], 16, 32)
    model.engine.set_tensor(100, g["U"])
    model.engine.set_tensor(101, g["V"])
    model.URM_train = model._URM_eval
    return model


def test_reference_golden_through_the_class_mf_contract(golden_dir):
    from ganmf_amd.evaluation import FULL_METRICS, EvaluatorNegativeItemSampleFast
    g = _golden(golden_dir)
    model = _golden_model(g, "mf")
    ev = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"],
                                         full_metrics=True)
    (res, _), calls = _counted(model, "evaluate_candidates_on_device", lambda: ev.evaluateRecommender(model))
    assert calls == 1
    for c, d in g["expected"].items():
        row = res[int(c)]
        assert list(row) == list(d) == list(FULL_METRICS)
        for key, want in d.items():
            if math.isnan(want):
                assert math.isnan(row[key]), (c, key)
            else:
                assert abs(row[key] - want) <= 1e-15 + 2e-5 * abs(want), (c, key, row[key], want)
    nine = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], minRatingsPerUser=g["min_ratings_per_user"])
    (res9, _), calls = _counted(model, "evaluate_candidates_on_device", lambda: nine.evaluateRecommender(model))
    assert calls == 1
    for c, d in g["expected"].items():
        for key in _SUM_BASED:
            assert abs(res9[int(c)][key] - d[key]) <= 1e-15 + 2e-5 * abs(d[key]), (c, key)
    # the explicit API on the same candidates: the reference's per-user lists
    items = model.recommend_candidates(np.arange(g["train"].shape[0]), ev.URM_items_to_rank, 8)
    assert np.all(items[6] == -1) and (items[7] >= 0).sum() == 2 and (items[5] >= 0).sum() == 3
    model.engine.close()


def test_ganmf_contract_declines_and_equals_holdout_fast(golden_dir):
    """score_contract="ganmf": items_to_compute is ignored as in the reference's GANMF, the device candidate route declines and
    the Fast class returns what EvaluatorHoldoutFast returns on the same inputs"""
    from ganmf_amd.evaluation import EvaluatorHoldoutFast, EvaluatorNegativeItemSampleFast
    g = _golden(golden_dir)
    model = _golden_model(g, "ganmf")
    assert not model.honours_items_to_compute
    for full in (False, True):
        kw = dict(minRatingsPerUser=g["min_ratings_per_user"], full_metrics=full)
        ev = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], **kw)
        assert model.evaluate_candidates_on_device(ev._device_token, ev._test_sorted, ev._test_gain, ev.URM_items_to_rank, ev._users,
                                                   ev.cutoff_list, ev._disc, ev._ideal_cum) is None
        fast, _ = ev.evaluateRecommender(model)
        hold, _ = EvaluatorHoldoutFast(g["test"], g["cutoffs"], **kw).evaluateRecommender(model)
        assert json.dumps(fast) == json.dumps(hold)
    model.engine.close()


def test_same_bytes_on_every_call_and_handle():
    rng = np.random.RandomState(41)
    nu, ni, k = 64, 700, 250
    U, V = rng.standard_normal((nu, k)).astype(np.float32), rng.standard_normal((ni, k)).astype(np.float32)
    cands = _lists(rng, nu, ni, [100, 257, 700])
    ids = rng.randint(0, nu, size=200)
    out = []
    for _ in range(2):
        eng = _engine(U, V)
        eng.set_candidates(_csr(cands, ni))
        for _ in range(2):
            items, vals = eng.recommend_candidates(ids, 50, remove_seen=False)
            out.append(items.tobytes() + vals.tobytes())
        eng.close()
    assert len(set(out)) == 1


def test_error_returns_leave_the_handle_usable():
    """argument checks only: each returns a negative code and a message without launching, and a valid call on the same
    handle succeeds afterwards"""
    from ganmf_amd._lib import CANDIDATES_MAX_PER_ROW as CMAX
    rng = np.random.RandomState(5)
    nu, ni, k = 12, CMAX + 20, 3
    U, V = _grid(rng, (nu, k)), _grid(rng, (ni, k))
    scores = U.astype(np.float64) @ V.astype(np.float64).T
    eng = _engine(U, V)
    ids = np.arange(4, dtype=np.int32)
    items = np.empty((4, 5), np.int32)
    vals = np.empty((4, 5), np.float32)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(rows, transposed=0):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        rc = eng.lib.ganmf_recommend_candidates(eng.h, rows.ctypes.data_as(i32p), rows.size, transposed, 5, 0,
                                                items.ctypes.data_as(i32p), vals.ctypes.data_as(f32p))
        return rc, (eng.lib.ganmf_last_error() or b"").decode()

    def valid(cands):
        rc, _ = call(ids)
        assert rc == 0
        np.testing.assert_array_equal(items, _expect([_ranked(scores[r], cands[r], []) for r in range(nu)], ids, 5)[0])

    rc, msg = call(ids)                                                   # no candidate matrix set
    assert rc < 0 and "candidate" in msg
    cands = _lists(rng, nu, ni, [30])
    eng.set_candidates(_csr(cands, ni))
    valid(cands)
    rc, msg = call(ids, transposed=1)                                     # a users x items matrix asked for in item mode
    assert rc < 0 and "transposed" in msg
    valid(cands)
    over = list(cands)
    over[9] = np.arange(CMAX + 1)                                         # one row over the limit: refused only when it is asked for
    eng.set_candidates(_csr(over, ni))
    rc, msg = call(np.array([1, 9, 2]))
    assert rc < 0 and "GANMF_CANDIDATES_MAX_PER_ROW" in msg
    valid(over)
    disc, ideal = np.ones(5), np.ones((4, 5))
    t = sps.csr_matrix((rng.rand(nu, ni) < 0.01).astype(np.float32))
    t.sort_indices()
    eng.set_test(t, np.ones(t.nnz))
    from ganmf_amd._lib import GanmfError
    with pytest.raises(GanmfError):                                       # the full row without ratings / weights, as ganmf_evaluate_full
        eng.evaluate_candidates(ids, [5], disc, ideal, remove_seen=False, full=True)
    with pytest.raises(GanmfError):                                       # more cut-offs than one call takes
        eng.evaluate_candidates(ids, list(range(1, 10)), np.ones(9), np.ones((4, 9)), remove_seen=False)
    assert eng.evaluate_candidates(ids, [5], disc, ideal, remove_seen=False).shape == (1, 9)
    eng.set_candidates(None)                                              # NULL clears
    rc, msg = call(ids)
    assert rc < 0 and "candidate" in msg
    eng.close()


def test_factors_too_long_for_the_lds_are_refused_without_a_launch():
    """padded factor rows longer than 512 floats live in LDS beside the candidate slots; past 144 KiB the call returns an
    error code and a message instead of launching"""
    rng = np.random.RandomState(9)
    nu, ni, k = 4, 70, 37000                       # 64 candidate slots (512 B) + 37 056 floats > 144 KiB
    U, V = _grid(rng, (nu, k)), _grid(rng, (ni, k))
    eng = _engine(U, V)
    eng.set_candidates(_csr(_lists(rng, nu, ni, [10]), ni))
    ids = np.arange(nu, dtype=np.int32)
    items, vals = np.empty((nu, 5), np.int32), np.empty((nu, 5), np.float32)
    rc = eng.lib.ganmf_recommend_candidates(eng.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), nu, 0, 5, 0,
                                            items.ctypes.data_as(C.POINTER(C.c_int32)), vals.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc < 0 and "LDS" in (eng.lib.ganmf_last_error() or b"").decode()
    eng.close()
