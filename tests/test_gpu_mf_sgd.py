"""MF-BPR and FunkSVD on the device (ganmf_mf_sgd_* on a GANMF_MODEL_MF handle) against the float64 restatement of
tests/helpers_mf_sgd.py and against what the reference's compiled epoch recorded (tests/golden/mf_sgd_tiny.npz).

Shapes: 70 users x 50 items of density 0.2 with one empty, one full and one all-but-one profile; num_factors 1, 10, 64, 65 and 250
(one lane; under, at and over one wave; four strides with a ragged last one).

Tolerance of the update tests.  The device and the restatement form the same real sums and products, every operation rounded once
(contraction is off in the kernels).  The restatement sums in the reference's order (R_seq) or in the device's documented one (R_tree:
lane-strided partial sums, an xor butterfly).  latitude = max |R_tree - R_seq| over a block of the state is the float64 re-ordering
latitude of that list, carried through it by the true dynamics.  The device is compared with R_tree under
    bound = 4 latitude + 1e-14 max |value|
The 4 covers the device's exp, sqrt and divisions, which may differ from the host's by an ulp: the same order as one re-ordering.
Lists are at most 3 epochs at learning_rate <= 0.05, so the latitude stays a rounding quantity.  Nothing in the bound is read from
the device.  Every case prints its latitude and the worst ratio error / bound (profiles/mf_sgd_fit.md)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_mf_sgd as H

pytestmark = pytest.mark.gpu

HP = dict(learning_rate=H.f32(0.03), user_reg=H.f32(0.02), positive_reg=H.f32(0.01), negative_reg=H.f32(0.005), bias_reg=H.f32(0.004))
CONFIGS = [("MF_BPR", False), ("FUNK_SVD", False), ("FUNK_SVD", True)]


def _urm(n_users=70, n_items=50, seed=0):
    rng = np.random.RandomState(seed)
    m = (rng.rand(n_users, n_items) < 0.2) * rng.randint(1, 6, size=(n_users, n_items))
    m[0] = 0                                          # empty: never drawn
    m[1] = rng.randint(1, 6, size=n_items)            # full: never drawn
    m[2] = rng.randint(1, 6, size=n_items)
    m[2, 33] = 0                                      # one possible negative: the fall-back after 64 refusals
    return sps.csr_matrix(m.astype(np.float64))


def _factors(urm, k, seed=1):
    rng = np.random.RandomState(seed)
    return rng.normal(0.0, 0.1, (urm.shape[0], k)), rng.normal(0.0, 0.1, (urm.shape[1], k))


def _rates(algorithm):
    names = ("learning_rate", "user_reg", "positive_reg", "negative_reg") if algorithm == "MF_BPR" else ("learning_rate", "user_reg", "positive_reg", "bias_reg")
    return {n: HP[n] for n in names}


def _engine(urm, algorithm, use_bias, mode, U0, V0, seed=0, quota=0.0, **rates):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(urm.shape[0], urm.shape[1], U0.shape[1] + 2 * int(use_bias), 1, 1, model=L.MODEL_MF)
    kw = _rates(algorithm)
    kw.update(rates)
    eng.mf_sgd_init(algorithm, urm, U0, V0, use_bias=use_bias, sgd_mode=mode, seed=seed, negative_interactions_quota=quota, **kw)
    return eng


def _trainer(algorithm, use_bias, mode, U0, V0, tree, **rates):
    kw = _rates(algorithm)
    kw.update(rates)
    return H.Trainer(algorithm, U0, V0, use_bias, mode, tree=tree, **kw)


def _same_state(a, b):
    return all(a[blk][n].tobytes() == b[blk][n].tobytes() for blk in ("params", "state0", "state1") for n in H.MEMBERS) and \
        a["beta_powers"].tobytes() == b["beta_powers"].tobytes()


def _check_against_restatement(state, seq, tree, label):
    """device against R_tree, block by block, under 4 latitude + 1e-14 max |value|"""
    worst = 0.0
    for blk, which in (("params", None), ("state0", 0), ("state1", 1)):
        a = seq.params() if which is None else seq.state(which)
        b = tree.params() if which is None else tree.state(which)
        latitude = max(np.abs(a[n] - b[n]).max() for n in H.MEMBERS)
        top = max(np.abs(b[n]).max() for n in H.MEMBERS)
        bound = 4.0 * latitude + 1e-14 * top
        err = max(np.abs(state[blk][n] - b[n]).max() for n in H.MEMBERS)
        ratio = err / bound if bound > 0 else 0.0
        print("%s %s: max |device - R_tree| %.3e, latitude %.3e, bound %.3e, ratio %.3f, max |value| %.3e" % (label, blk, err, latitude, bound, ratio, top))
        assert err <= bound, (label, blk, err, bound)
        worst = max(worst, ratio)
    assert np.array_equal(state["beta_powers"], [tree.b1p, tree.b2p])      # formed on the host by the same multiplications
    return worst


def _list(algorithm, urm, k):
    """at most 3 epochs; fewer samples for the wide models, which cost the restatement most"""
    epochs = 1 if algorithm == "FUNK_SVD" else (3 if k <= 10 else 2)      # (a FunkSVD epoch is 768 samples, an MF-BPR one 72)
    return H.draw(algorithm, 17, 0, epochs, urm, 8, quota=0.3)


# ---- the update against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64, 65, 250])
@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("algorithm,use_bias", CONFIGS)
def test_injected_lists_against_the_restatement(algorithm, use_bias, mode, k):
    from ganmf_amd import _lib as L
    urm = _urm()
    U0, V0 = _factors(urm, k)
    samples = _list(algorithm, urm, k)
    seq = _trainer(algorithm, use_bias, mode, U0, V0, False).apply(*samples, batch_size=8)
    tree = _trainer(algorithm, use_bias, mode, U0, V0, True).apply(*samples, batch_size=8)
    a, b = _engine(urm, algorithm, use_bias, mode, U0, V0), _engine(urm, algorithm, use_bias, mode, U0, V0)
    assert a.mf_sgd_run(*samples, batch_size=8, route=L.MF_SGD_SEQUENTIAL) == 0
    levels = b.mf_sgd_run(*samples, batch_size=8, route=L.MF_SGD_LEVELLED)
    assert 1 <= levels <= 8
    sa, sb = a.mf_sgd_state(), b.mf_sgd_state()
    assert _same_state(sa, sb)      # the two routes, byte for byte
    _check_against_restatement(sa, seq, tree, "%s bias=%s %s k=%d" % (algorithm, use_bias, mode, k))
    assert np.abs(sa["params"]["USER_factors"] - U0).max() > 1e-4      # (the list did train something)
    assert (sa["state1"]["USER_factors"].any()) == (mode == "adam") and (sa["state0"]["USER_factors"].any()) == (mode != "sgd")
    assert sa["params"]["GLOBAL_bias"].any() == use_bias and sa["params"]["ITEM_bias"].any() == use_bias
    a.close()
    b.close()


def _conflict_lists(urm):
    """(users, items, neg_items) lists whose consecutive samples share the user only, the positive only, and in which one sample's
    negative is the next one's positive; and one in which user 5 is in every sample"""
    n = 8
    ids = np.arange(n + 1) + 10
    return {"shared user": (np.full(n, 4), np.arange(n), np.arange(n) + 20),
            "shared positive": (np.arange(n) + 3, np.full(n, 7), np.arange(n) + 20),
            "j becomes i": (np.arange(n) + 3, ids[:n], ids[1:]),
            "one row in every sample": (np.full(n, 5), np.arange(n) * 2, np.arange(n) * 2 + 1)}


@pytest.mark.parametrize("mode", ["sgd", "adam"])
@pytest.mark.parametrize("algorithm,use_bias", CONFIGS)
def test_conflict_lists_and_batch_sizes_on_both_routes(algorithm, use_bias, mode):
    from ganmf_amd import _lib as L
    urm = _urm()
    U0, V0 = _factors(urm, 10)
    rng = np.random.RandomState(3)
    for name, (users, items, neg) in _conflict_lists(urm).items():
        third = neg if algorithm == "MF_BPR" else rng.randint(0, 6, users.size).astype(np.float64)
        for batch_size, want in ((1, 1), (8, None), (50, None)):      # 50: larger than the list
            a, b = _engine(urm, algorithm, use_bias, mode, U0, V0), _engine(urm, algorithm, use_bias, mode, U0, V0)
            a.mf_sgd_run(users, items, third, batch_size, route=L.MF_SGD_SEQUENTIAL)
            levels = b.mf_sgd_run(users, items, third, batch_size, route=L.MF_SGD_AUTO)      # AUTO: levelled
            if want is None:
                chained = name != "j becomes i" or algorithm == "MF_BPR"      # FunkSVD has no j: nothing is shared
                want = 8 if chained else 1
            assert levels == want, (name, batch_size, levels)      # one row in every sample: as many levels as the batch has samples
            sa, sb = a.mf_sgd_state(), b.mf_sgd_state()
            assert _same_state(sa, sb), (name, batch_size)
            seq = _trainer(algorithm, use_bias, mode, U0, V0, False).apply(users, items, third, batch_size)
            tree = _trainer(algorithm, use_bias, mode, U0, V0, True).apply(users, items, third, batch_size)
            _check_against_restatement(sa, seq, tree, "%s bias=%s %s %s batch %d" % (algorithm, use_bias, mode, name, batch_size))
            # a second call continues from the first (the beta powers carry on), on the other route
            a.mf_sgd_run(users, items, third, batch_size, route=L.MF_SGD_LEVELLED)
            b.mf_sgd_run(users, items, third, batch_size, route=L.MF_SGD_SEQUENTIAL)
            assert _same_state(a.mf_sgd_state(), b.mf_sgd_state()), (name, batch_size, "second call")
            a.close()
            b.close()


def test_two_runs_return_the_same_bytes():
    urm = _urm()
    U0, V0 = _factors(urm, 65)
    samples = H.draw("FUNK_SVD", 3, 0, 1, urm, 16, quota=0.3)
    states = []
    for _ in range(2):
        eng = _engine(urm, "FUNK_SVD", True, "adam", U0, V0)
        eng.mf_sgd_run(*samples, batch_size=16)
        states.append(eng.mf_sgd_state())
        eng.close()
    assert _same_state(*states)


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm,quota", [("MF_BPR", 0.0), ("FUNK_SVD", 0.0), ("FUNK_SVD", 0.3), ("FUNK_SVD", 0.999)])
def test_sampler_equals_its_restatement_and_respects_the_profiles(algorithm, quota):
    urm = _urm()
    dense = urm.toarray()
    U0, V0 = _factors(urm, 4)
    eng = _engine(urm, algorithm, False, "sgd", U0, V0, seed=99, quota=quota)
    n_epochs = 8 if algorithm == "MF_BPR" else 2
    got = eng.mf_sgd_draw(0, n_epochs, batch_size=8)
    want = H.draw(algorithm, 99, 0, n_epochs, urm, 8, quota=quota)
    per = H.per_epoch(algorithm, urm, 8)
    assert got[0].size == n_epochs * per and got[0].dtype == np.int32
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    users, items, third = got
    assert not np.any(np.isin(users, [0, 1]))      # never the empty or the full user
    assert np.any(users == 2)
    if algorithm == "MF_BPR":
        assert np.all(dense[users, items] > 0) and np.all(dense[users, third] == 0)
        assert set(third[users == 2]) == {33}      # mostly through the fall-back after 64 refusals
    else:
        assert np.all(third == dense[users, items])      # a positive carries its rating, a negative 0 and lies outside the profile
        share = np.mean(third > 0)
        assert share == 1.0 if quota == 0.0 else (0.2 < share < 0.4 if quota == 0.3 else share > 0.99)
        if quota == 0.3:
            assert set(items[(users == 2) & (third == 0)]) == {33}
    # addressed by epoch, and nothing of the state moved
    e1 = eng.mf_sgd_draw(1, 1, batch_size=8)
    assert all(np.array_equal(a, b[per:2 * per]) for a, b in zip(e1, got))
    state = eng.mf_sgd_state()
    assert state["epoch"] == 0 and np.array_equal(state["params"]["USER_factors"], U0)
    other = _engine(urm, algorithm, False, "sgd", U0, V0, seed=100, quota=quota)
    assert not np.array_equal(other.mf_sgd_draw(0, 1, batch_size=8)[0], users[:per])
    assert eng.mf_sgd_draw(5, 0, batch_size=8)[0].size == 0
    eng.close()
    other.close()


def test_mf_bpr_and_slim_bpr_draw_the_same_triples():
    """there is ONE sampler (draw_kernel of counter_draw.hpp): with the same profiles, the same seed and the same samples per epoch
    -- SLIM-BPR's is num_users + 1, MF-BPR's at batch_size = num_users + 1 is (num_users // batch_size + 1) * batch_size, the same --
    the two entries return the same arrays"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = _urm(40, 70)
    U0, V0 = _factors(urm, 4)
    mf = _engine(urm, "MF_BPR", False, "sgd", U0, V0, seed=31)
    slim = Engine(40, 70, 1, 1, 1, model=L.MODEL_ITEMSIM)
    slim.slim_bpr_init(symmetric=False, sgd_mode="sgd", seed=31, profiles=sps.csr_matrix(urm, dtype=np.float32))
    a, b = mf.mf_sgd_draw(0, 2, batch_size=41), slim.slim_bpr_draw(0, 2)
    assert a[0].size == b[0].size == 2 * 41
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.int32 and np.array_equal(x, y)
    assert len(set(a[0])) > 10 and not np.any(np.isin(a[0], [0, 1]))      # (a real draw: many users, never the empty or the full one)
    mf.close()
    slim.close()


@pytest.mark.parametrize("algorithm,use_bias", CONFIGS)
def test_epochs_is_draw_followed_by_run(algorithm, use_bias):
    from ganmf_amd import _lib as L
    urm = _urm()
    U0, V0 = _factors(urm, 10)
    for route in (L.MF_SGD_AUTO, L.MF_SGD_SEQUENTIAL):
        a, b = (_engine(urm, algorithm, use_bias, "adam", U0, V0, seed=8, quota=0.3) for _ in range(2))
        levels = a.mf_sgd_epochs(2, batch_size=16, route=route)
        assert (levels >= 1) == (route == L.MF_SGD_AUTO)
        a.mf_sgd_epochs(1, batch_size=16, route=route)
        b.mf_sgd_run(*b.mf_sgd_draw(0, 3, batch_size=16), batch_size=16, route=L.MF_SGD_SEQUENTIAL)
        sa, sb = a.mf_sgd_state(), b.mf_sgd_state()
        assert _same_state(sa, sb) and sa["epoch"] == 3 and sb["epoch"] == 0
        # set_state: a third handle resumes from the read-back and lands on the same bytes
        c = _engine(urm, algorithm, use_bias, "adam", U0, V0, seed=8, quota=0.3)
        c.mf_sgd_set_state(sa["params"], sa["state0"], sa["state1"], sa["beta_powers"], sa["epoch"])
        a.mf_sgd_epochs(1, batch_size=16, route=route)
        c.mf_sgd_epochs(1, batch_size=16, route=route)
        assert _same_state(a.mf_sgd_state(), c.mf_sgd_state()) and c.mf_sgd_state()["epoch"] == 4
        for e in (a, b, c):
            e.close()


# ---- the reference's recorded runs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mf_sgd_tiny.npz"), allow_pickle=False)


@pytest.mark.parametrize("n", range(12))
def test_fixture_lists_against_the_reference_s_finals(golden, n):
    """the list the reference drew (predicted from its seed), injected from its initial factors: the device against the finals the
    compiled epoch left, under 4 |R_tree - reference| + 1e-14 max |value| per member"""
    p = json.loads(str(golden["c%d_params" % n]))
    urm = sps.csr_matrix((golden["urm_data"], golden["urm_indices"], golden["urm_indptr"]), shape=tuple(golden["urm_shape"]))
    rates = dict(learning_rate=H.f32(p["learning_rate"]), user_reg=H.f32(p["user_reg"]))
    if p["algorithm"] == "MF_BPR":
        rates.update(positive_reg=H.f32(p["positive_reg"]), negative_reg=H.f32(p["negative_reg"]))
    else:
        rates.update(bias_reg=H.f32(p["bias_reg"]), positive_reg=0.0)
    U0, V0 = golden["c%d_U0" % n], golden["c%d_V0" % n]
    samples = tuple(golden["c%d_%s" % (n, k)] for k in ("users", "items", "third"))
    eng = _engine(urm, p["algorithm"], p["use_bias"], p["sgd_mode"], U0, V0, **rates)
    eng.mf_sgd_run(*samples, batch_size=8)
    got = eng.mf_sgd_state()["params"]
    eng.close()
    tree = H.Trainer(p["algorithm"], U0, V0, p["use_bias"], p["sgd_mode"], tree=True, **rates).apply(*samples, batch_size=8).params()
    for name in (H.MEMBERS if p["use_bias"] else H.MEMBERS[:2]):
        ref = golden["c%d_%s" % (n, name)]
        latitude = np.abs(tree[name].reshape(ref.shape) - ref).max()
        bound = 4.0 * latitude + 1e-14 * np.abs(ref).max()
        err = np.abs(got[name].reshape(ref.shape) - ref).max()
        print("fixture case %d %s %s bias=%s quota=%s %s: max |device - reference| %.3e, latitude %.3e, bound %.3e, ratio %.3f" % (
            n, p["algorithm"], p["sgd_mode"], p["use_bias"], p["quota"], name, err, latitude, bound, err / bound))
        assert err <= bound, (name, err, bound)


# ---- the classes ------------------------------------------------------------------------------------------------------------------------------
def _split(seed=1):
    rng = np.random.RandomState(seed)
    urm = sps.csr_matrix(_urm(), dtype=np.float32)
    dense = urm.toarray()
    dense[6] = 0      # a cold user
    test = sps.csr_matrix(((dense == 0) * (rng.rand(*dense.shape) < 0.15)).astype(np.float32))
    return sps.csr_matrix(dense), test


def _counted(model, name):
    inner, got = getattr(model, name), []

    def wrapper(*a, **kw):
        got.append(inner(*a, **kw))
        return got[-1]
    setattr(model, name, wrapper)
    return got


@pytest.mark.parametrize("cls_name,use_bias", [("MatrixFactorization_BPR_Cython", False), ("MatrixFactorization_FunkSVD_Cython", False),
                                               ("MatrixFactorization_FunkSVD_Cython", True)])
def test_publish_scores_and_the_device_routes_of_the_class(cls_name, use_bias, tmp_path):
    import MatrixFactorization.Cython.MatrixFactorization_Cython as M
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    urm, test = _split()
    model = getattr(M, cls_name)(urm)
    try:
        model.fit(epochs=3, batch_size=16, num_factors=7, learning_rate=0.05, use_bias=use_bias, sgd_mode="adagrad", user_reg=0.01,
                  bias_reg=0.01, negative_interactions_quota=0.3, random_seed=4)
        assert model.epochs_best == 2 and model.use_bias is use_bias and model.USER_factors.dtype == np.float64
        assert model.USER_factors.shape == (70, 7) and model.engine.shape(100) == (70, 7 + 2 * use_bias)
        # scores = the float64 U V^T + ITEM_bias + GLOBAL_bias + USER_bias[u] of the class's own read-back
        want = model.USER_factors @ model.ITEM_factors.T
        if use_bias:
            want = want + model.ITEM_bias[None, :] + float(model.GLOBAL_bias) + model.USER_bias[:, None]
            assert np.abs(model.ITEM_bias).max() > 0 and np.abs(model.USER_bias).max() > 0 and float(model.GLOBAL_bias) != 0.0
        scores = model._compute_item_score(np.arange(70))
        warm = np.flatnonzero(np.diff(urm.indptr) > 0)
        assert np.isneginf(scores[6]).all() and 6 not in warm      # the cold-user mask, as IALSRecommender
        for u in warm:
            assert np.abs(scores[u] - want[u]).max() <= 1e-5 * np.abs(scores[u]).max(), u
        # the evaluator, recommend and the activity study take the model through the device routes
        hook = _counted(model, "evaluate_on_device")
        results, _ = EvaluatorHoldoutFast(test, [5]).evaluateRecommender(model)
        assert len(hook) >= 1 and all(r is not None for r in hook) and 0.0 <= results[5]["MAP"] <= 1.0
        groups = _counted(model, "evaluate_groups_on_device")
        study = model.activity_study(test, [3, 10], cutoff=5)
        assert len(groups) >= 1 and all(r is not None for r in groups) and np.nansum(study["n_users"]) > 0
        lists = model.recommend([3, 6, 7], cutoff=5)
        assert lists[1] == [] and len(lists[0]) == 5 and not set(lists[0]) & set(urm[3].indices)
        masked = np.where(urm.toarray() > 0, -np.inf, want)
        assert np.allclose(np.sort(masked[3])[::-1][:5], masked[3, lists[0]], rtol=1e-4, atol=1e-6)
        # saveModel -> a fresh instance's loadModel -> the same score bytes
        before = model._compute_item_score(warm)
        model.saveModel(str(tmp_path))
        other = getattr(M, cls_name)(urm)
        other.loadModel(str(tmp_path))
        assert other.use_bias is use_bias and np.array_equal(other._compute_item_score(warm), before)
        other.engine.close()
    finally:
        model.engine.close()


class _Evaluator(object):
    def __init__(self, values):
        self.values, self.seen = list(values), []

    def evaluateRecommender(self, model):
        self.seen.append((model._compute_item_score(np.arange(10, 20)), model.USER_factors.copy()))
        return {5: {"MAP": self.values[len(self.seen) - 1]}}, ""


def test_best_slot_is_restored_after_a_worse_epoch():
    from MatrixFactorization.Cython.MatrixFactorization_Cython import MatrixFactorization_FunkSVD_Cython
    urm, _ = _split()
    model = MatrixFactorization_FunkSVD_Cython(urm)
    ev = _Evaluator([0.2, 0.5, 0.1])
    model.fit(epochs=3, batch_size=16, num_factors=5, learning_rate=0.05, random_seed=2, validation_every_n=1, validation_metric="MAP",
              evaluator_object=ev)
    assert model.epochs_best == 2 and model.best_validation_metric == 0.5
    assert not np.array_equal(ev.seen[1][0], ev.seen[2][0])
    assert np.array_equal(model._compute_item_score(np.arange(10, 20)), ev.seen[1][0])      # the tensors came back from the best slot
    assert np.array_equal(model.USER_factors, ev.seen[1][1])
    last = model.engine.mf_sgd_state()
    assert last["epoch"] == 3 and not np.array_equal(last["params"]["USER_factors"], model.USER_factors)
    model.engine.close()


def _planted(seed=5):
    rng = np.random.RandomState(seed)
    P, Q = rng.normal(size=(70, 3)), rng.normal(size=(50, 3))
    S = P @ Q.T
    return sps.csr_matrix((S > np.quantile(S, 0.8)).astype(np.float32)), S


def test_training_signal_on_a_planted_matrix():
    """deterministic under the fixed seed: after 30 BPR epochs the training-pair AUC exceeds that of the initial factors; FunkSVD's
    mean squared error on the stored ratings falls"""
    from MatrixFactorization.Cython.MatrixFactorization_Cython import MatrixFactorization_BPR_Cython, MatrixFactorization_FunkSVD_Cython
    urm, S = _planted()
    dense = urm.toarray() > 0

    def auc(U, V):
        scores = U @ V.T
        vals = []
        for u in range(70):
            pos, neg = scores[u, dense[u]], scores[u, ~dense[u]]
            if pos.size and neg.size:
                vals.append(np.mean(pos[:, None] > neg[None, :]))
        return float(np.mean(vals))

    model = MatrixFactorization_BPR_Cython(urm)
    model.fit(epochs=30, batch_size=8, num_factors=3, learning_rate=0.05, sgd_mode="adagrad", random_seed=3)
    rng = np.random.RandomState(3)
    U0, V0 = rng.normal(0.0, 0.1, (70, 3)), rng.normal(0.0, 0.1, (50, 3))
    before, after = auc(U0, V0), auc(model.USER_factors, model.ITEM_factors)
    print("MF_BPR training-pair AUC: %.4f -> %.4f after 30 epochs" % (before, after))
    assert after > before
    model.engine.close()

    ratings = sps.csr_matrix(urm.multiply(np.clip(np.round(S + 3.0), 1, 5)).astype(np.float32))
    r = ratings.tocoo()

    def mse(m):
        pred = np.sum(m.USER_factors[r.row] * m.ITEM_factors[r.col], axis=1) + m.USER_bias[r.row] + m.ITEM_bias[r.col] + float(m.GLOBAL_bias)
        return float(np.mean((r.data - pred) ** 2))

    errs = []
    for epochs in (1, 30):
        funk = MatrixFactorization_FunkSVD_Cython(ratings)
        funk.fit(epochs=epochs, batch_size=8, num_factors=3, learning_rate=0.05, sgd_mode="adagrad", random_seed=3)
        errs.append(mse(funk))
        funk.engine.close()
    print("FUNK_SVD mean squared error on the stored ratings: %.4f after 1 epoch -> %.4f after 30" % tuple(errs))
    assert errs[1] < errs[0]


# ---- error paths ------------------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_handle_usable():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = _urm()
    U0, V0 = _factors(urm, 4)
    eng = Engine(70, 50, 4, 1, 1, model=L.MODEL_MF)
    ok = (np.array([3]), np.array([int(urm[3].indices[0])]), np.array([int(np.setdiff1d(np.arange(50), urm[3].indices)[0])]))
    for name in ("ganmf_mf_sgd_publish", "ganmf_mf_sgd_epochs"):
        rc = eng.lib.ganmf_mf_sgd_publish(eng.h) if name.endswith("publish") else eng.lib.ganmf_mf_sgd_epochs(eng.h, 1, 8, 0, None)
        assert rc == -1 and b"ganmf_mf_sgd_init has not been called" in eng.lib.ganmf_last_error()
    with pytest.raises(ValueError, match="sgd_mode"):
        eng.mf_sgd_init("MF_BPR", urm, U0, V0, sgd_mode="momentum")
    with pytest.raises(ValueError, match="algorithm_name"):
        eng.mf_sgd_init("ASY_SVD", urm, U0, V0)
    with pytest.raises(ValueError, match="profiles must be 70 x 50"):
        eng.mf_sgd_init("MF_BPR", sps.csr_matrix((70, 51)), U0, V0)
    with pytest.raises(ValueError, match="initial factors must be"):
        eng.mf_sgd_init("FUNK_SVD", urm, U0, V0, use_bias=True)      # 4 columns would leave 2 factors
    with pytest.raises(L.GanmfError, match=r"\(-1\).*must be finite"):
        eng.mf_sgd_init("MF_BPR", urm, U0, V0, learning_rate=float("nan"))
    with pytest.raises(L.GanmfError, match=r"\(-1\).*quota must be in \[0, 1\)"):
        eng.mf_sgd_init("FUNK_SVD", urm, U0, V0, negative_interactions_quota=1.0)
    with pytest.raises(L.GanmfError, match=r"\(-1\).*MF_BPR has no biases"):
        eng.mf_sgd_init("MF_BPR", urm, U0[:, :2], V0[:, :2], use_bias=True)
    bad = U0.copy()
    bad[5, 1] = np.inf
    with pytest.raises(L.GanmfError, match=r"\(-1\).*initial user factors are not finite"):
        eng.mf_sgd_init("MF_BPR", urm, bad, V0)
    unsorted = sps.csr_matrix(urm, copy=True)
    lo = unsorted.indptr[4]
    unsorted.indices[lo:lo + 2] = unsorted.indices[lo:lo + 2][::-1].copy()
    with pytest.raises(L.GanmfError, match="not sorted"):
        eng.mf_sgd_init("MF_BPR", unsorted, U0, V0)
    nobody = np.zeros((70, 50))
    nobody[1] = nobody[3] = 1
    with pytest.raises(L.GanmfError, match=r"\(-1\).*neither empty nor full"):
        eng.mf_sgd_init("MF_BPR", sps.csr_matrix(nobody), U0, V0)
    with pytest.raises(L.GanmfError, match="has not been called"):      # still no state after the refusals
        eng.mf_sgd_state()
    eng.mf_sgd_init("MF_BPR", urm, U0, V0, learning_rate=0.05)
    # a refused init keeps the state held
    with pytest.raises(L.GanmfError, match="must be finite"):
        eng.mf_sgd_init("MF_BPR", urm, U0, V0, user_reg=float("inf"))
    for bad_list, what in (((np.array([70]), ok[1], ok[2]), "names user 70 of 70"), ((ok[0], np.array([50]), ok[2]), "names item 50 of 50"),
                           ((ok[0], ok[1], np.array([-1])), "names item -1"), ((ok[0], ok[1], ok[1]), "same positive and negative")):
        with pytest.raises(L.GanmfError, match=r"\(-1\).*" + what):
            eng.mf_sgd_run(*bad_list, batch_size=8)
    with pytest.raises(L.GanmfError, match="unknown route"):
        eng.mf_sgd_run(*ok, batch_size=8, route=7)
    for batch_size in (0, (1 << 20) + 1):
        with pytest.raises(L.GanmfError, match=r"batch_size must be in \[1, 1048576\]"):
            eng.mf_sgd_run(*ok, batch_size=batch_size)
        with pytest.raises(L.GanmfError, match=r"batch_size must be in \[1, 1048576\]"):
            eng.mf_sgd_epochs(1, batch_size=batch_size)
    with pytest.raises(L.GanmfError, match="must be >= 0"):
        eng.mf_sgd_draw(-1, 1, batch_size=8)
    with pytest.raises(L.GanmfError, match="must be >= 0"):
        eng.mf_sgd_epochs(-1, batch_size=8)
    state = eng.mf_sgd_state()
    poisoned = {k: v.copy() for k, v in state["params"].items()}
    poisoned["ITEM_factors"][0, 0] = np.nan
    with pytest.raises(L.GanmfError, match="not finite"):
        eng.mf_sgd_set_state(params=poisoned)
    assert np.array_equal(eng.mf_sgd_state()["params"]["USER_factors"], U0)      # nothing was enqueued by a refused call
    assert eng.mf_sgd_run(np.zeros(0), np.zeros(0), np.zeros(0), batch_size=8) == 0      # an empty list is allowed
    eng.mf_sgd_run(*ok, batch_size=8)
    eng.mf_sgd_publish()
    after = eng.mf_sgd_state()["params"]
    assert not np.array_equal(after["USER_factors"][3], U0[3]) and np.array_equal(after["USER_factors"][4], U0[4])
    assert np.array_equal(eng.get_tensor(L.T_USER_EMB), after["USER_factors"].astype(np.float32))
    funk = Engine(70, 50, 4, 1, 1, model=L.MODEL_MF)
    funk.mf_sgd_init("FUNK_SVD", urm, U0, V0)
    with pytest.raises(L.GanmfError, match="rating that is not finite"):
        funk.mf_sgd_run(ok[0], ok[1], np.array([np.nan]), batch_size=8)
    funk.close()
    eng.close()
    sim = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM)
    with pytest.raises(L.GanmfError, match="GANMF_MODEL_MF"):
        sim.mf_sgd_init("MF_BPR", urm, U0[:, :1], V0[:, :1])
    sim.close()

