"""ganmf_evaluate_groups -- per-user hold-out metrics and their sums per group of users on the device -- through the C ABI, the
evaluators' evaluateRecommenderByGroup and the user-activity study (ganmf_amd/studies.py).

Exact rankings: factors on the grid {-1, -3/4, ..., 1} with k = 8, so every score is exact in fp32 in any order and the host can
form the device's lists itself (score descending, ties to the smaller id).  The per-user values are then float64 on both sides
and differ only in the order of a handful of additions and in j * (1 / rank) against j / rank: 1e-12 * max(1, |v|), the figure
tests/test_gpu_recommend.py holds the device sums to against the host."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

ROWS, WIDTH, K_FACTORS, CUTOFFS = 600, 70, 8, [1, 5, 20]
TIDS = (0, 1, 2, 3, 100, 101)


def _close(got, want, what=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = ~(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert not bad.any(), (what, got[bad][:4], want[bad][:4])


def _grid(rng, shape):
    return (rng.randint(-4, 5, size=shape) / 4.0).astype(np.float32)


class _Case(object):
    """one engine per orientation with its seen / test matrices, and the host's per-user values of all 600 rows, formed once"""

    def __init__(self, transposed):
        from ganmf_amd._lib import EVAL_METRICS
        from ganmf_amd.evaluation import EvaluatorHoldoutFast, RankedListMetrics
        rng = np.random.RandomState(17 + transposed)
        self.transposed = bool(transposed)
        self.rows_f, self.cols_f = _grid(rng, (ROWS, K_FACTORS)), _grid(rng, (WIDTH, K_FACTORS))
        scores = self.rows_f.astype(np.float64) @ self.cols_f.astype(np.float64).T
        seen = rng.rand(ROWS, WIDTH) < 0.3
        seen[::7] = rng.rand(len(seen[::7]), WIDTH) < 0.85                 # every seventh row keeps ~10 unseen items: lists below 20
        t = ((rng.rand(ROWS, WIDTH) < 0.08) * rng.randint(1, 6, size=(ROWS, WIDTH))).astype(np.float32)
        t[np.arange(ROWS), rng.randint(0, WIDTH, ROWS)] = 3.0              # every row has a test item (RECALL is a number)
        self.seen, self.test = sps.csr_matrix(seen.astype(np.float32)), sps.csr_matrix(t)
        self.ev = EvaluatorHoldoutFast(self.test, CUTOFFS)
        assert len(self.ev._users) == ROWS
        self.want = np.zeros((ROWS, len(CUTOFFS), 9))
        short = 0
        for r in range(ROWS):
            s = np.where(seen[r], -np.inf, scores[r])
            order = np.lexsort((np.arange(WIDTH), -s))
            order = order[np.isfinite(s[order])][:max(CUTOFFS)]
            short += len(order) < max(CUTOFFS)
            scorer = RankedListMetrics(self.ev.get_user_relevant_items(r), self.ev.get_user_test_ratings(r), max(CUTOFFS), dtype=np.float64)
            hit, gain = scorer.match(order)
            for ci, c in enumerate(CUTOFFS):
                row = scorer(hit, gain, c)
                self.want[r, ci] = [row[m] for m in EVAL_METRICS]
        assert short > 20 and self.want[:, 2, 4].max() > 0.25 and (self.want[:, 2, 7] == 0).any()
        self.engine = self.new_engine()

    def new_engine(self):
        from ganmf_amd.engine import Engine
        eng = (Engine(WIDTH, ROWS, K_FACTORS, 16, 32) if self.transposed else Engine(ROWS, WIDTH, K_FACTORS, 16, 32))
        eng.set_tensor(100, self.cols_f if self.transposed else self.rows_f)
        eng.set_tensor(101, self.rows_f if self.transposed else self.cols_f)
        eng.set_seen(self.seen)
        eng.set_test(self.ev._test_sorted, self.ev._test_gain)
        return eng

    def groups(self, ids, group_of, n_groups, eng=None, **kw):
        return (eng or self.engine).evaluate_groups(ids, CUTOFFS, self.ev._disc, self.ev._ideal_cum[ids], group_of, n_groups,
                                                    transposed=self.transposed, **kw)


@pytest.fixture(scope="module", params=[False, True], ids=["user", "item"])
def case(request):
    c = _Case(request.param)
    yield c
    c.engine.close()


def _group_of(rng, n, G):
    """group per position with -1 entries; G = 3: group 1 stays empty, G = 256: group 200 does"""
    g = rng.randint(-1, G, size=n)
    if G > 1:
        g[g == (1 if G == 3 else 200)] = -1
    return g


@pytest.mark.parametrize("G", [1, 3, 256])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_per_user_values_group_sums_and_sizes(case, n, G):
    """n at the block edges of the 256-thread kernels, ids a shuffled subset; G = 1, 3 and GANMF_EVAL_MAX_GROUPS with an empty
    group and -1 entries"""
    from ganmf_amd._lib import EVAL_MAX_GROUPS
    assert EVAL_MAX_GROUPS == 256
    rng = np.random.RandomState(1000 * G + n)
    ids = rng.permutation(ROWS)[:n]
    group_of = _group_of(rng, n, G)
    sums, sizes, per_user = case.groups(ids, group_of, G, per_user=True)
    assert sums.shape == (G, 3, 9) and sizes.shape == (G,) and per_user.shape == (n, 3, 9)
    _close(per_user, case.want[ids], (n, G))
    for g in range(G):
        assert sizes[g] == int((group_of == g).sum())                       # exact
        _close(sums[g], per_user[group_of == g].sum(axis=0, dtype=np.float64), (n, G, g))
    if G > 1:
        empty = 1 if G == 3 else 200
        assert sizes[empty] == 0 and not sums[empty].any()
    assert sizes.sum() == int((group_of >= 0).sum()) and (n < 20 or (group_of == -1).any())
    # without per_user, and per-user values alone (no groups): the same bytes
    sums2, sizes2, none = case.groups(ids, group_of, G)
    assert none is None and sums2.tobytes() == sums.tobytes() and sizes2.tobytes() == sizes.tobytes()
    _, _, alone = case.groups(ids, None, 0, per_user=True)
    assert alone.tobytes() == per_user.tobytes()


@pytest.mark.parametrize("remove_seen", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_one_group_of_everyone_equals_ganmf_evaluate(case, n, remove_seen):
    rng = np.random.RandomState(n)
    ids = rng.permutation(ROWS)[:n]
    want = case.engine.evaluate(ids, CUTOFFS, case.ev._disc, case.ev._ideal_cum[ids], transposed=case.transposed, remove_seen=remove_seen)
    sums, sizes, _ = case.groups(ids, np.zeros(n, np.int32), 1, remove_seen=remove_seen)
    assert sizes.tolist() == [n]
    _close(sums[0], want, (n, remove_seen))
    assert want[2, 7] > 0 or n == 1


def test_same_bytes_on_every_call_and_handle(case):
    rng = np.random.RandomState(5)
    ids = rng.permutation(ROWS)[:513]
    group_of = _group_of(rng, len(ids), 3)
    out = []
    other = case.new_engine()
    for eng in (case.engine, other):
        for _ in range(2):
            sums, sizes, per_user = case.groups(ids, group_of, 3, eng=eng, per_user=True)
            out.append(sums.tobytes() + sizes.tobytes() + per_user.tobytes())
    other.close()
    assert len(set(out)) == 1


def test_no_side_effects(case):
    """parameters, Adam moments and powers are the bytes they were; ganmf_evaluate before and after gives the same bytes"""
    eng = case.engine
    rng = np.random.RandomState(9)
    ids = rng.permutation(ROWS)[:300]

    def state():
        return b"".join(eng.get_tensor(t, slot).tobytes() for t in TIDS for slot in (0, 1, 2)) + eng.adam_powers().tobytes()

    def evaluate():
        return eng.evaluate(ids, CUTOFFS, case.ev._disc, case.ev._ideal_cum[ids], transposed=case.transposed).tobytes()

    before, ev_before = state(), evaluate()
    case.groups(ids, _group_of(rng, len(ids), 256), 256, per_user=True)
    case.groups(ids[:7], None, 0, per_user=True)
    assert state() == before and evaluate() == ev_before


def test_error_returns_leave_the_handle_usable(case):
    """argument checks only: each returns -1 and a message without a launch, and the next valid call succeeds"""
    from ganmf_amd._lib import EVAL_MAX_GROUPS
    eng = case.new_engine()
    n = 40
    ids = np.arange(n, dtype=np.int32)
    cut = np.asarray(CUTOFFS, dtype=np.int32)
    disc = np.ascontiguousarray(case.ev._disc, dtype=np.float64)
    ideal = np.ascontiguousarray(case.ev._ideal_cum[ids], dtype=np.float64)
    sums = np.zeros((EVAL_MAX_GROUPS + 1, 3, 9))
    sizes = np.zeros(EVAL_MAX_GROUPS + 1, dtype=np.int64)
    users = np.zeros((n, 3, 9))
    i32p, dp, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def call(group_of, n_groups, want_sums=True, want_users=True, candidates=0, h=eng):
        g = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.int32)
        rc = h.lib.ganmf_evaluate_groups(h.h, ids.ctypes.data_as(i32p), n, int(case.transposed), 1, candidates, cut.ctypes.data_as(i32p), 3,
                                         disc.ctypes.data_as(dp), ideal.ctypes.data_as(dp), None if g is None else g.ctypes.data_as(i32p),
                                         n_groups, sums.ctypes.data_as(dp) if want_sums else None,
                                         sizes.ctypes.data_as(i64p) if want_sums else None, users.ctypes.data_as(dp) if want_users else None)
        return rc, (h.lib.ganmf_last_error() or b"").decode()

    def valid(h=eng):
        users[:] = -1.0
        rc, _ = call(np.arange(n) % 3, 3, h=h)
        assert rc == 0 and sizes[:3].tolist() == [14, 13, 13]
        _close(users, case.want[ids])

    zeros = np.zeros(n, np.int32)
    valid()
    for bad in (lambda: call(zeros, EVAL_MAX_GROUPS + 1),                   # too many groups
                lambda: call(np.where(np.arange(n) == 5, 3, 0), 3),         # an entry equal to n_groups
                lambda: call(np.where(np.arange(n) == 39, -2, 0), 3),       # an entry below -1
                lambda: call(None, 0, want_sums=False, want_users=False),   # neither output asked for
                lambda: call(zeros, 1, candidates=1)):                      # candidates without a candidate matrix
        rc, msg = bad()
        assert rc == -1 and "ganmf_evaluate_groups" in msg, (rc, msg)
        valid()
    rc, msg = call(zeros, -1)
    assert rc == -1 and "groups" in msg
    eng.close()
    from ganmf_amd.engine import Engine
    bare = Engine(WIDTH, ROWS, K_FACTORS, 16, 32) if case.transposed else Engine(ROWS, WIDTH, K_FACTORS, 16, 32)
    bare.set_seen(case.seen)
    rc, msg = call(zeros, 1, h=bare)                                        # no test matrix set
    assert rc == -1 and "ganmf_set_test_csr" in msg
    bare.set_tensor(100, case.cols_f if case.transposed else case.rows_f)
    bare.set_tensor(101, case.rows_f if case.transposed else case.cols_f)
    bare.set_test(case.ev._test_sorted, case.ev._test_gain)
    valid(h=bare)
    bare.close()


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


def _same_groups(dev, host, cutoffs):
    from ganmf_amd._lib import EVAL_METRICS
    assert sorted(dev) == sorted(host)
    for label in host:
        assert dev[label]["n_users"] == host[label]["n_users"]
        for c in cutoffs:
            assert list(dev[label][c]) == list(host[label][c]) == list(EVAL_METRICS) + ["F1"]
            for name, v in host[label][c].items():
                _close(dev[label][c][name], v, (label, c, name))


def _factor_model(g, contract="ganmf"):
    from ganmf_amd.GANMF import GANMF
    model = GANMF(g["train"], mode="user", is_experiment=True, score_contract=contract)
    model._build(g["U"].shape[1], 16, 32)
    model.engine.set_tensor(100, g["U"])
    model.engine.set_tensor(101, g["V"])
    model.URM_train = model._URM_eval
    return model


def _load(golden_dir, name):
    g = json.load(open(os.path.join(golden_dir, name)))
    for key in ("train", "test", "negative"):
        g[key] = sps.csr_matrix(np.array(g[key], np.float32))
    g["U"], g["V"] = np.array(g["U"], np.float32), np.array(g["V"], np.float32)
    return g


def test_candidates_route_equals_the_host_negative_sample_evaluators(golden_dir):
    """the inputs of the reference's negative-sample golden under score_contract="mf": ganmf_evaluate_groups with candidates = 1
    against the grouped host routes (the Fast class's, and the reference-order class through recommend(items_to_compute=...))"""
    from ganmf_amd.evaluation import EvaluatorNegativeItemSample, EvaluatorNegativeItemSampleFast
    g = _load(golden_dir, "negative_sample_expected.json")
    model = _factor_model(g, "mf")
    n_users = g["train"].shape[0]
    groups = np.arange(n_users) % 4 - 1                                     # -1, 0, 1, 2
    groups[groups == 1] = 5                                                 # labels need not be dense
    kw = dict(minRatingsPerUser=g["min_ratings_per_user"])
    ev = EvaluatorNegativeItemSampleFast(g["test"], g["negative"], g["cutoffs"], **kw)
    (dev, dev_users, ids), calls = _counted(model, "evaluate_groups_on_device",
                                            lambda: ev.evaluateRecommenderByGroup(model, groups, return_per_user=True))
    assert calls == 1 and sorted(dev) == [0, 2, 5]
    ev._block_size = 5
    blocks, calls = _counted(model, "evaluate_groups_on_device", lambda: ev.evaluateRecommenderByGroup(model, groups))
    assert calls == -(-len(ev._users) // 5)
    ev._block_size = None
    ev.use_device_metrics = False
    host, host_users, host_ids = ev.evaluateRecommenderByGroup(model, groups, return_per_user=True)
    slow = EvaluatorNegativeItemSample(g["test"], g["negative"], g["cutoffs"], **kw).evaluateRecommenderByGroup(model, groups)
    _same_groups(dev, host, g["cutoffs"])
    _same_groups(blocks, host, g["cutoffs"])
    _same_groups(dev, slow, g["cutoffs"])
    assert ids.tolist() == host_ids.tolist()
    _close(dev_users, host_users)
    assert host[0][5]["MAP"] > 0
    # the reference's GANMF contract declines the candidate route, as evaluate_candidates_on_device does
    plain = _factor_model(g, "ganmf")
    assert plain.evaluate_groups_on_device(ev._device_token, ev._test_sorted, ev._test_gain, ev._users, ev.cutoff_list, ev._disc,
                                           ev._ideal_cum, np.zeros(len(ev._users), np.int32), 1,
                                           candidates_csr=ev.URM_items_to_rank) is None
    plain.engine.close()
    model.engine.close()


def _fitted(kind, urm):
    from ganmf_amd.DisGANMF import DisGANMF
    from ganmf_amd.GANMF import GANMF
    if kind == "disganmf":
        m = DisGANMF(urm, mode="user", seed=4, is_experiment=True)
        m.fit(num_factors=5, d_layers=1, d_nodes=8, d_hidden_act="tanh", epochs=1, batch_size=16)
    else:
        m = GANMF(urm, mode="item" if kind == "ganmf_item_mf" else "user", seed=3, is_experiment=True,
                  score_contract="mf" if kind == "ganmf_item_mf" else None)
        m.fit(num_factors=5, emb_dim=8, epochs=1, batch_size=16)
    return m


@pytest.mark.parametrize("kind", ["ganmf_user", "ganmf_item_mf", "disganmf"])
def test_through_the_classes(golden_dir, kind):
    """one epoch on the tiny matrix: activity_study and EvaluatorHoldoutFast.evaluateRecommenderByGroup on the device against
    the evaluator's host route (lists from recommend_topk, metrics from RankedListMetrics)"""
    from ganmf_amd._lib import EVAL_METRICS
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    from ganmf_amd.studies import activity_bucket, activity_bucket_keys
    urm = sps.load_npz(os.path.join(golden_dir, "tiny_urm.npz")).tocsr()
    rng = np.random.RandomState(23)
    nu, ni = urm.shape
    t = ((rng.rand(nu, ni) < 0.15) * rng.randint(1, 6, size=(nu, ni))).astype(np.float32)
    t[urm.toarray() != 0] = 0
    t[:3] = 0                                                               # users without a test item
    test = sps.csr_matrix(t)
    model = _fitted(kind, urm)
    bounds = [22, 28, 36]                                                   # (a user with count 22 sits on the first bound)
    cutoffs = [1, 5, 20]
    counts = np.asarray((urm + test).sum(axis=1)).reshape(-1)
    groups = activity_bucket(counts, bounds)
    assert len(set(groups[3:])) == 4
    ev = EvaluatorHoldoutFast(test, cutoffs)
    (dev, dev_users, ids), calls = _counted(model, "evaluate_groups_on_device",
                                            lambda: ev.evaluateRecommenderByGroup(model, groups, return_per_user=True))
    assert calls == 1
    ev.use_device_metrics = False
    host, host_users, _ = ev.evaluateRecommenderByGroup(model, groups, return_per_user=True)
    _same_groups(dev, host, cutoffs)
    _close(dev_users, host_users)
    study = model.activity_study(test, bounds, cutoff=20)
    keys, plotted = activity_bucket_keys(bounds)
    assert study["keys"] == keys == ["<22", ">=22, <28", ">=28, <36", ">=36"] and study["plotted"] == plotted == [True, True, False, True]
    assert study["skipped"] == 3 and np.isnan(study["per_user"][:3]).all() and study["per_user"].shape == (nu,)
    _close(study["per_user"][ids], host_users[:, 2, EVAL_METRICS.index("MAP")])
    for b in range(4):
        assert study["n_users"][b] == host[b]["n_users"] > 0
        _close(study["means"][b], host[b][20]["MAP"], (kind, b))
    assert np.array_equal(study["bucket"], groups) and np.nanmax(study["per_user"]) > 0
    ndcg = model.activity_study(test, bounds, cutoff=5, metric="NDCG")
    _close(ndcg["per_user"][ids], host_users[:, 1, EVAL_METRICS.index("NDCG")])
    with pytest.raises(RuntimeError):                                       # device route only: no host fallback
        model.activity_study(test, bounds, cutoff=ni + 1)
    model.engine.close()


def test_reference_golden_through_the_device_route(golden_dir):
    """tests/golden/activity_study_expected.json: the reference's recommend + average_precision per user, through
    activity_study on the device"""
    g = _load(golden_dir, "activity_study_expected.json")
    model = _factor_model(g)
    who = g["users"]
    for c in g["cutoffs"]:
        want = np.array([np.nan if v is None else v for v in g["ap"][str(c)]])
        study, calls = _counted(model, "evaluate_groups_on_device", lambda: model.activity_study(g["test"], g["bounds"], cutoff=c))
        assert calls == 1 and study["skipped"] == len(who["no_test"]) == int(np.isnan(want).sum())
        assert np.array_equal(np.isnan(study["per_user"]), np.isnan(want))
        ok = ~np.isnan(want)
        _close(study["per_user"][ok], want[ok], c)
        assert study["keys"] == ["<8", ">=8, <16", ">=16, <30", ">=30, <50", ">=50"] and study["plotted"] == [True, True, True, False, True]
        assert study["bucket"][who["on_bound"]] == 2 and study["bucket"][who["short_list"]] == 4
        for b in range(5):
            members = ok & (study["bucket"] == b)
            assert study["n_users"][b] == members.sum() > 0
            _close(study["means"][b], want[members].sum() / members.sum(), (c, b))
    assert study["per_user"][who["no_hit"]] == 0.0
    model.engine.close()
