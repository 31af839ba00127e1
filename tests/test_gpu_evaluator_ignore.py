"""ignore_items / ignore_users / diversity_object on the device: the ignore list of ganmf_set_items_to_ignore in everything that
ranks, ganmf_evaluate_diversity (list_diversity.hpp) and the evaluators' device routes around them -- against rows recorded from the
reference's evaluators (tests/golden/evaluator_ignore_*), against the host routes of the same model, and at the entry points."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.evaluation import (BEYOND_ACCURACY, METRICS, EvaluatorHoldoutFast, EvaluatorNegativeItemSampleFast,
                                  list_diversity)

pytestmark = pytest.mark.gpu

DIV = "DIVERSITY_SIMILARITY"


def _close(got, want, rtol, what):
    if math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= 1e-15 + rtol * abs(want), (what, got, want)


def _counted(model, hooks, call):
    """call() with every named hook of the model counted and required to take the device route"""
    n = dict.fromkeys(hooks, 0)

    def wrap(name, orig):
        def counted(*a, **k):
            n[name] += 1
            out = orig(*a, **k)
            assert out is not None, name
            return out
        return counted
    for name in hooks:
        setattr(model, name, wrap(name, getattr(model, name)))
    try:
        out = call()
    finally:
        for name in hooks:
            delattr(model, name)
    return out, n


def _host_rows(ev, model):
    ev.use_device_metrics = False
    try:
        return ev.evaluateRecommender(model)[0]
    finally:
        ev.use_device_metrics = True


def _model(mode, n_users, n_items, k, seed, density=0.08, cls=None, **kw):
    from ganmf_amd.GANMF import GANMF
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_users, n_items) < density).astype(np.float32)
    m[np.arange(n_users), rng.randint(0, n_items, n_users)] = 1.0
    urm = sps.csr_matrix(m)
    model = (cls or GANMF)(urm, mode=mode, is_experiment=True, **kw)
    model._build(k, 16, 32)
    model.engine.set_tensor(100, rng.randn(model.num_users, k).astype(np.float32))
    model.engine.set_tensor(101, rng.randn(model.num_items, k).astype(np.float32))
    model.URM_train = model._URM_eval
    return model, urm, rng


def _quantised(rng, n):
    """an asymmetric diversity matrix with entries q / 256: every partial sum is exact in float64, whatever the order"""
    return (rng.randint(0, 257, size=(n, n)) / 256.0).astype(np.float32)


# ---- the reference's rows through the device route ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "evaluator_ignore_inputs.npz"))
    g = json.load(open(os.path.join(golden_dir, "evaluator_ignore_expected.json")))
    return dict(train=sps.csr_matrix(z["train"].astype(np.float32)), U=z["U"], V=z["V"],
                test=sps.csr_matrix(z["test"].astype(np.float32)), negative=sps.csr_matrix(z["negative"].astype(np.float32)),
                D=z["D"].astype(np.float64) / 256.0, ignore_items=z["ignore_items"], ignore_users=z["ignore_users"],
                cutoffs=g["cutoffs"], min_ratings=g["min_ratings_per_user"], expected=g["expected"])


def _fixture_model(fx, mode, **kw):
    from ganmf_amd.GANMF import GANMF
    model = GANMF(fx["train"], mode=mode, is_experiment=True, **kw)
    model._build(fx["U"].shape[1], 16, 32)
    # evaluation users' factors: the generator's rows in user mode, its columns in item mode
    model.engine.set_tensor(100, fx["U"] if mode == "user" else fx["V"])
    model.engine.set_tensor(101, fx["V"] if mode == "user" else fx["U"])
    model.URM_train = model._URM_eval
    return model


def _check_golden(res, exp, full, what):
    for c, d in exp.items():
        row = res[int(c)]
        if full:
            assert list(row) == list(d), (what, c, list(row))
        else:
            assert set(row) == set(METRICS) | ({DIV} & set(d)) and list(row)[-1] == (DIV if DIV in d else "F1"), (what, c, list(row))
        for k in row:
            if k == "RMSE" and not full:
                assert math.isnan(row[k])
                continue
            _close(row[k], d[k], 1e-9 if k in BEYOND_ACCURACY or k == DIV else 2e-5, (what, c, k))


@pytest.mark.parametrize("mode", ["user", "item"])
@pytest.mark.parametrize("full", [True, False])
def test_reference_rows_through_the_device_route(fx, mode, full):
    model = _fixture_model(fx, mode)
    for name, kw in (("holdout_all", dict(diversity_object=fx["D"], ignore_items=fx["ignore_items"], ignore_users=fx["ignore_users"])),
                     ("holdout_diversity", dict(diversity_object=fx["D"])),
                     ("holdout_ignore_items", dict(ignore_items=fx["ignore_items"])),
                     ("holdout_ignore_users", dict(ignore_users=fx["ignore_users"]))):
        ev = EvaluatorHoldoutFast(fx["test"], fx["cutoffs"], minRatingsPerUser=fx["min_ratings"], full_metrics=full, **kw)
        ev._block_size = 100
        hooks = ["evaluate_full_on_device" if full else "evaluate_on_device"] + (["evaluate_diversity_on_device"] if "diversity_object" in kw else [])
        (res, _), n = _counted(model, hooks, lambda: ev.evaluateRecommender(model))
        assert all(v == -(-len(ev._users) // 100) for v in n.values()), n
        _check_golden(res, fx["expected"][name], full, (mode, name))
        assert not model.items_to_ignore_flag
    model.engine.close()


@pytest.mark.parametrize("full", [True, False])
def test_reference_negative_sample_row_through_the_candidate_route(fx, full):
    model = _fixture_model(fx, "user", score_contract="mf")
    assert np.ediff1d(fx["train"].indptr).min() > 0                    # nobody is cold: the MF contract masks nothing else
    ev = EvaluatorNegativeItemSampleFast(fx["test"], fx["negative"], fx["cutoffs"], minRatingsPerUser=fx["min_ratings"], full_metrics=full,
                                         diversity_object=fx["D"], ignore_users=fx["ignore_users"])
    (res, _), n = _counted(model, ["evaluate_candidates_on_device", "evaluate_diversity_on_device"], lambda: ev.evaluateRecommender(model))
    assert set(n.values()) == {1}
    _check_golden(res, fx["expected"]["negative_users_diversity"], full, "negative")
    model.engine.close()


# ---- device route against the host route of the same model (both rank the same device scores) ------------------------------------
def _same_rows(dev, host, cutoffs, what):
    for c in cutoffs:
        assert list(dev[c]) == list(host[c]), (what, c)
        for k in dev[c]:
            _close(dev[c][k], host[c][k], 2e-6 if k == "RMSE" else 1e-12, (what, c, k))


@pytest.fixture(scope="module")
def wide():
    """300 x 203 (no multiple of 64), k = 12, with a graded test matrix, an ignore list and a diversity matrix"""
    out = {}
    for mode in ("user", "item"):
        model, urm, rng = _model(mode, 300, 203, 12, seed=21)
        t = ((rng.rand(300, 203) < 0.06) * rng.randint(1, 6, size=(300, 203))).astype(np.float32)
        t[rng.rand(300) < 0.1] = 0
        out[mode] = dict(model=model, urm=urm, test=sps.csr_matrix(t), D=_quantised(rng, 203),
                         ignore_items=np.concatenate([rng.choice(203, 31, replace=False), [5, 5]]),
                         ignore_users=rng.choice(300, 40, replace=False))
    yield out
    for mode in out:
        out[mode]["model"].engine.close()


@pytest.mark.parametrize("mode", ["user", "item"])
@pytest.mark.parametrize("exclude_seen", [True, False])
@pytest.mark.parametrize("case", ["ignore", "diversity", "all"])
def test_device_route_equals_host_route(wide, mode, exclude_seen, case):
    w = wide[mode]
    kw = {}
    if case in ("ignore", "all"):
        kw["ignore_items"] = w["ignore_items"]
    if case in ("diversity", "all"):
        kw["diversity_object"] = w["D"]
    if case == "all":
        kw["ignore_users"] = w["ignore_users"]
    cut = [2, 5, 20]
    for full in (True, False):
        ev = EvaluatorHoldoutFast(w["test"], cut, exclude_seen=exclude_seen, full_metrics=full, **kw)
        hooks = ["evaluate_full_on_device" if full else "evaluate_on_device"] + (["evaluate_diversity_on_device"] if "diversity_object" in kw else [])
        (dev, _), n = _counted(w["model"], hooks, lambda: ev.evaluateRecommender(w["model"]))
        assert set(n.values()) == {1}
        host = _host_rows(ev, w["model"])
        _same_rows(dev, host, cut, (mode, case, full, "one block"))
        assert (DIV in dev[5]) == ("diversity_object" in kw)
        if full:
            dev_full = dev
        ev._block_size = 37
        (blocks, _), n = _counted(w["model"], hooks, lambda: ev.evaluateRecommender(w["model"]))
        assert set(n.values()) == {-(-len(ev._users) // 37)}
        _same_rows(blocks, host, cut, (mode, case, full, "blocks of 37"))
    if case != "diversity":
        plain = EvaluatorHoldoutFast(w["test"], cut, exclude_seen=exclude_seen, full_metrics=True).evaluateRecommender(w["model"])[0]
        assert plain[20]["MAP"] != dev_full[20]["MAP"] and dev_full[20]["COVERAGE_ITEM"] <= (203 - 31) / (203 - 33)


def test_short_lists_on_the_device(wide):
    """all but 8 items ignored: L_c = len below the cut-off; a user with exactly one unmasked item and one with none (L_c < 2 -> 0,
    still counted in the mean)"""
    w = wide["user"]
    model, seen = w["model"], w["urm"].toarray() != 0
    unseen_count = (~seen).sum(axis=0)
    keep = np.argsort(-unseen_count, kind="stable")[:8]
    ignore = np.setdiff1d(np.arange(203), keep)
    train = w["urm"].tolil(copy=True)
    one, none = 7, 19
    train[one, keep[1:]] = 1.0
    train[one, keep[0]] = 0.0
    train[none, keep] = 1.0
    m2, _, _ = _model("user", 300, 203, 12, seed=21)
    m2._URM_eval = m2.URM_train = sps.csr_matrix(train, dtype=np.float32)
    m2.engine.set_seen(m2._URM_eval)
    t = w["test"].tolil(copy=True)
    t[one, 3] = 2.0
    t[none, 4] = 5.0
    cut = [2, 5, 20]
    ev = EvaluatorHoldoutFast(sps.csr_matrix(t), cut, full_metrics=True, ignore_items=ignore, diversity_object=w["D"])
    (dev, _), n = _counted(m2, ["evaluate_full_on_device", "evaluate_diversity_on_device"], lambda: ev.evaluateRecommender(m2))
    host = _host_rows(ev, m2)
    _same_rows(dev, host, cut, "short lists")
    assert dev[5][DIV] > 0 and dev[20]["COVERAGE_USER"] < 1.0
    m2.set_items_to_ignore(ignore)
    with m2._ignored_items(True):
        sums, users = m2.engine.evaluate_diversity(ev._users, cut, per_user=True)
        lists, _ = m2.engine.recommend(ev._users, 20)
    m2.reset_items_to_ignore()
    assert (lists >= 0).sum(axis=1).max() == 8 and not set(lists[lists >= 0].tolist()) - set(keep.tolist())
    at = {u: i for i, u in enumerate(ev._users.tolist())}
    assert (lists[at[one]] >= 0).sum() == 1 and (lists[at[none]] >= 0).sum() == 0
    assert np.all(users[at[one]] == 0.0) and np.all(users[at[none]] == 0.0)
    want = list_diversity(w["D"], lists, cut)
    assert np.array_equal(users, want)                       # entries q / 256: exact sums, the same rounding of the one division
    long_enough = (lists >= 0).sum(axis=1) == 8
    assert np.array_equal(users[long_enough][:, 2], list_diversity(w["D"], lists[long_enough][:, :8], [8])[:, 0])   # L_c = len
    m2.engine.close()


@pytest.mark.parametrize("candidates", [False, True])
def test_long_lists_take_several_passes(candidates):
    """K = 256: every wave walks 64 list rows in four column passes; cut-offs given out of order, one of them twice"""
    model, urm, rng = _model("user", 70, 333, 12, seed=5, score_contract="mf")
    eng = model.engine
    D = _quantised(rng, 333)
    eng.set_item_diversity(D)
    ignore = rng.choice(333, 17, replace=False)
    cut = [100, 256, 7, 100, 64, 65]
    users = rng.permutation(70)[:50].astype(np.int32)
    if candidates:
        cand = (rng.rand(70, 333) < 0.95).astype(np.float32)
        cand[3] = 0                                           # a user with two candidates
        cand[3, [8, 200]] = 1
        eng.set_candidates(sps.csr_matrix(cand))
    eng.set_items_to_ignore(ignore)
    rank = eng.recommend_candidates if candidates else eng.recommend
    lists, _ = rank(users, 256)
    sums, per_user = eng.evaluate_diversity(users, cut, candidates=candidates, per_user=True)
    eng.set_items_to_ignore(None)
    assert (lists >= 0).sum(axis=1).max() == 256 and not set(lists[lists >= 0].tolist()) & set(ignore.tolist())
    want = list_diversity(D, lists, cut)
    assert np.array_equal(per_user, want)                      # entries q / 256: exact sums, the same two roundings of the division
    assert np.array_equal(per_user[:, 0], per_user[:, 3]) and want.max() > 0
    _close(sums.sum(), want.sum(), 1e-12, "sums")
    eng.close()


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_ignore_list_composes_with_the_mf_filter_and_the_cold_mask():
    model, urm, rng = _model("user", 90, 203, 12, seed=9, score_contract="mf")
    train = urm.tolil(copy=True)
    train[11] = 0                                                # a cold user
    model._URM_eval = model.URM_train = sps.csr_matrix(train, dtype=np.float32)
    model.engine.set_seen(model._URM_eval)
    eng = model.engine
    compute = rng.choice(203, 120, replace=False)
    ignore = np.concatenate([compute[:25], np.setdiff1d(np.arange(203), compute)[:10]])
    users = np.arange(90, dtype=np.int32)
    eng.set_score_filter(compute, mask_cold=True)
    filtered = eng.scores(users)
    eng.set_items_to_ignore(ignore)
    assert np.array_equal(eng.scores(users), filtered)           # ganmf_scores keeps the plain filter
    items, vals = eng.recommend(users, 30, remove_seen=True)
    eng.set_score_filter(None, mask_cold=True)                   # the filter goes, the ignore list stays
    items_nofilter, _ = eng.recommend(users, 30, remove_seen=True)
    eng.set_items_to_ignore(None)
    items_plain, _ = eng.recommend(users, 30, remove_seen=True)
    unfiltered = eng.scores(users)

    def host(scores, masked):
        s = scores.copy()
        s[:, np.asarray(masked, dtype=np.int64)] = -np.inf
        s[model._URM_eval.toarray() != 0] = -np.inf
        order = np.lexsort((np.arange(203)[None, :].repeat(90, 0), -s), axis=1)[:, :30]
        return np.where(np.isfinite(np.take_along_axis(s, order, axis=1)), order, -1)
    assert np.array_equal(items, host(filtered, ignore))
    assert np.array_equal(items_nofilter, host(unfiltered, ignore))
    assert np.array_equal(items_plain, host(unfiltered, []))
    assert np.all(items[11] == -1) and (items[0] >= 0).all() and set(items[items >= 0].tolist()) <= set(compute[25:].tolist())
    eng.close()


def test_scores_and_similarity_do_not_see_the_ignore_list(wide):
    eng = wide["item"]["model"].engine
    ids = np.arange(0, 203, 3, dtype=np.int32)
    scores, sim = eng.scores(ids, transposed=True), eng.score_similarity(ids, transposed=True, return_matrix=True)
    eng.set_items_to_ignore(np.arange(0, 203, 7))
    try:
        scores2, sim2 = eng.scores(ids, transposed=True), eng.score_similarity(ids, transposed=True, return_matrix=True)
        lists, _ = eng.recommend(ids, 10, transposed=True, remove_seen=False)
    finally:
        eng.set_items_to_ignore(None)
    assert scores.tobytes() == scores2.tobytes() and sim["matrix"].tobytes() == sim2["matrix"].tobytes()
    assert (sim["sum_d"], sim["sum_d2"]) == (sim2["sum_d"], sim2["sum_d2"]) and np.isfinite(scores).all()
    assert not (lists % 7 == 0).any()


@pytest.mark.parametrize("mode", ["user", "item"])
def test_recommend_flags_stay_on_the_device(wide, mode):
    w = wide[mode]
    model = w["model"]
    users = np.arange(0, 300, 2)
    model.set_items_to_ignore(w["ignore_items"])
    model.filterTopPop_ItemsID = np.argsort(-np.asarray(w["urm"].sum(axis=0)).ravel(), kind="stable")[:9]
    try:
        for flags in (dict(remove_CustomItems_flag=True), dict(remove_top_pop_flag=True),
                      dict(remove_CustomItems_flag=True, remove_top_pop_flag=True)):
            host, _ = model.recommend(users, cutoff=20, return_scores=True, **flags)       # the host route: full score matrix
            scores = model.engine.scores

            def no_scores(*a, **k):
                raise AssertionError("the device route does not fetch the score matrix")
            model.engine.scores = no_scores
            try:
                dev = model.recommend(users, cutoff=20, **flags)
                topk = model.recommend_topk(users, 20, **flags)
                one = model.recommend(int(users[3]), cutoff=20, **flags)
            finally:
                model.engine.scores = scores
            assert dev == host and one == host[3] and [r[r >= 0].tolist() for r in topk] == host
            masked = set()
            if flags.get("remove_CustomItems_flag"):
                masked |= set(w["ignore_items"].tolist())
            if flags.get("remove_top_pop_flag"):
                masked |= set(model.filterTopPop_ItemsID.tolist())
            assert not set(np.concatenate(dev).tolist()) & masked
        plain = model.recommend(users, cutoff=20)
        assert set(np.concatenate(plain).tolist()) & set(w["ignore_items"].tolist())      # the list is gone after each call
    finally:
        model.reset_items_to_ignore()
        model.filterTopPop_ItemsID = np.array([], dtype=int)


def test_ignore_list_is_cleared_after_the_evaluation(wide):
    w = wide["user"]
    model = w["model"]
    users = np.arange(300)
    before = model.recommend(users, cutoff=20)
    ev = EvaluatorHoldoutFast(w["test"], [5, 20], full_metrics=True, ignore_items=w["ignore_items"], diversity_object=w["D"])
    ev.evaluateRecommender(model)
    assert not model.items_to_ignore_flag and len(model.items_to_ignore_ID) == 0
    assert model.recommend(users, cutoff=20) == before
    assert set(np.concatenate(before).tolist()) & set(w["ignore_items"].tolist())
    grouped = ev.evaluateRecommenderByGroup(model, np.arange(300) % 2)
    assert model.recommend(users, cutoff=20) == before and grouped[0][20]["MAP"] >= 0


def test_disganmf_through_the_device_route():
    from ganmf_amd.DisGANMF import DisGANMF
    rng = np.random.RandomState(2)
    urm = sps.csr_matrix((rng.rand(120, 67) < 0.1).astype(np.float32))
    model = DisGANMF(urm, mode="user", seed=4, is_experiment=True)
    model.fit(num_factors=8, d_nodes=16, epochs=1, batch_size=32)
    test = sps.csr_matrix(((rng.rand(120, 67) < 0.15) * rng.randint(1, 6, size=(120, 67))).astype(np.float32))
    ev = EvaluatorHoldoutFast(test, [2, 5, 20], full_metrics=True, diversity_object=_quantised(rng, 67),
                              ignore_items=rng.choice(67, 9, replace=False), ignore_users=[3, 4, 50])
    (dev, _), n = _counted(model, ["evaluate_full_on_device", "evaluate_diversity_on_device"], lambda: ev.evaluateRecommender(model))
    assert set(n.values()) == {1}
    _same_rows(dev, _host_rows(ev, model), [2, 5, 20], "DisGANMF")
    model.engine.close()


def test_sharded_engine_equals_single_engine_twin():
    sh, urm, rng = _model("user", 150, 71, 8, seed=8, dist_backend="local", world_size=2)
    assert type(sh.engine).__name__ == "ShardedEngine"
    twin, _, _ = _model("user", 150, 71, 8, seed=8)
    test = sps.csr_matrix(((rng.rand(150, 71) < 0.15) * rng.randint(1, 6, size=(150, 71))).astype(np.float32))
    D, ignore = _quantised(rng, 71), rng.choice(71, 11, replace=False)
    ev = EvaluatorHoldoutFast(test, [2, 5, 20], full_metrics=True, diversity_object=D, ignore_items=ignore, ignore_users=[1, 2, 3])
    hooks = ["evaluate_full_on_device", "evaluate_diversity_on_device"]
    (a, _), _ = _counted(sh, hooks, lambda: ev.evaluateRecommender(sh))
    (b, _), _ = _counted(twin, hooks, lambda: ev.evaluateRecommender(twin))
    _same_rows(a, b, [2, 5, 20], "sharded vs single")
    sh.set_items_to_ignore(ignore)
    twin.set_items_to_ignore(ignore)
    assert sh.recommend(np.arange(150), cutoff=10, remove_CustomItems_flag=True) == twin.recommend(np.arange(150), cutoff=10,
                                                                                                   remove_CustomItems_flag=True)
    sh.engine.close()
    twin.engine.close()


def test_evaluate_diversity_is_reproducible_and_sums_its_rows(wide):
    eng = wide["user"]["model"].engine
    rng = np.random.RandomState(3)
    D = rng.rand(203, 203).astype(np.float32)                 # arbitrary float32 entries: the order of the sums matters here
    eng.set_item_diversity(D)
    users = rng.permutation(300).astype(np.int32)              # two workgroups of the user sum
    cut = [20, 3, 50]
    s1, u1 = eng.evaluate_diversity(users, cut, per_user=True)
    s2, u2 = eng.evaluate_diversity(users, cut, per_user=True)
    s3 = eng.evaluate_diversity(users, cut)
    assert s1.tobytes() == s2.tobytes() == s3.tobytes() and u1.tobytes() == u2.tobytes()
    for ci in range(3):
        _close(u1[:, ci].sum(), s1[ci], 1e-12, ci)
    lists, _ = eng.recommend(users, 50)
    want = list_diversity(D, lists, cut)
    assert np.abs(u1 - want).max() <= 1e-12 * want.max() and want.min() > 0


def test_entry_points_reject_bad_input():
    from ganmf_amd._lib import load_library
    model, urm, rng = _model("user", 40, 30, 4, seed=3)
    eng, lib = model.engine, load_library()
    ids = np.arange(6, dtype=np.int32)
    cut = np.array([2, 5], dtype=np.int32)
    sums = np.zeros(2)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))     # noqa: E731
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))    # noqa: E731

    def diversity(ids=ids, cut=cut, n_cut=2, sums=sums, transposed=0):
        return lib.ganmf_evaluate_diversity(eng.h, i32(ids), ids.size, transposed, 1, 0, i32(cut), n_cut,
                                            f64(sums) if sums is not None else None, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.ganmf_last_error().decode(), (rc, lib.ganmf_last_error())

    refused(diversity(), "no diversity matrix")
    eng.set_item_diversity(np.full((40, 40), 0.5, dtype=np.float32))
    refused(diversity(), "width 40")                                        # a matrix of the other orientation's width
    eng.set_item_diversity(np.full((30, 30), 0.5, dtype=np.float32))
    refused(diversity(sums=None), "null argument")
    refused(diversity(n_cut=0), "cut-offs per call")
    refused(diversity(cut=np.arange(1, 10, dtype=np.int32), n_cut=9), "cut-offs per call")
    refused(diversity(cut=np.array([2, 31], dtype=np.int32)), "cutoff 31 out of range")
    bad = np.array([3, 40], dtype=np.int32)
    refused(lib.ganmf_set_items_to_ignore(eng.h, i32(bad), 2), "item 40 out of range")
    wide_id = np.array([35], dtype=np.int32)                                # inside max(U, N), outside the 30 score columns
    assert lib.ganmf_set_items_to_ignore(eng.h, i32(wide_id), 1) == 0
    refused(diversity(), "ignore list lists item 35")
    out = np.zeros((6, 5), dtype=np.int32)
    refused(lib.ganmf_recommend(eng.h, i32(ids), 6, 0, 5, 1, i32(out), None), "ignore list lists item 35")
    assert lib.ganmf_set_items_to_ignore(eng.h, None, 0) == 0
    # the handle is usable; every pair is 0.5 and L - 1 of the L rows are visited: 0.5 (L - 1) / L per user
    assert diversity() == 0 and np.allclose(sums, [6 * 0.25, 6 * 0.4], rtol=1e-14)
    eng.set_item_diversity(None)
    refused(diversity(), "no diversity matrix")
    eng.close()
