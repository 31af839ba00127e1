"""MF-BPR and FunkSVD without a device: the float64 restatement (tests/helpers_mf_sgd.py) against cases worked out by hand and against
what the reference's compiled epoch recorded (tests/golden/mf_sgd_tiny.npz), and the host logic of the MatrixFactorization_*_Cython classes on a
helper engine.  (The level scheduler: tests/test_level_sched_host.py.)"""
import json
import math
import os
import zipfile

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_mf_sgd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the update, by hand ---------------------------------------------------------------------------------------------------------------
def test_bpr_batch_of_two_by_hand():
    W, Hm = [[0.5, -1.0]], [[1.0, 2.0], [0.0, 1.0], [3.0, 0.0]]
    t = H.Trainer("MF_BPR", W, Hm, learning_rate=0.25, user_reg=0.5, positive_reg=0.125, negative_reg=0.0625)
    t.apply([0, 0], [0, 1], [1, 2], batch_size=2)
    x0 = 0.5 * (1.0 - 0.0) + -1.0 * (2.0 - 1.0)
    x1 = 0.5 * (0.0 - 3.0) + -1.0 * (1.0 - 0.0)
    s = (1.0 / (1.0 + math.exp(x0)) + 1.0 / (1.0 + math.exp(x1))) / 2.0
    assert t.scalars == [s]      # one scalar for the batch, formed before anything moves
    # sample 0, factor 0: reads the initial rows
    w, hi, hj = 0.5, 1.0, 0.0
    w1 = w + 0.25 * (s * (hi - hj) - 0.5 * w)
    assert t.H[0][0] == hi + 0.25 * (s * w - 0.125 * hi)
    # sample 1 reads the rows sample 0 left: item 1 was its negative, user 0 its user
    h1 = hj + 0.25 * (s * (-w) - 0.0625 * hj)
    assert t.W[0][0] == w1 + 0.25 * (s * (h1 - 3.0) - 0.5 * w1)
    assert t.H[1][0] == h1 + 0.25 * (s * w1 - 0.125 * h1)
    assert t.H[2][0] == 3.0 + 0.25 * (s * (-w1) - 0.0625 * 3.0)


def test_funk_batch_with_biases_by_hand():
    t = H.Trainer("FUNK_SVD", [[1.0], [2.0]], [[0.5], [0.25]], use_bias=True, learning_rate=0.5, user_reg=0.25, positive_reg=0.0, bias_reg=0.125)
    t.apply([0, 1], [0, 0], [3.0, 1.0], batch_size=2)
    s = ((3.0 - 0.5) + (1.0 - 1.0)) / 2.0
    assert t.scalars == [s] and t.gb == [0.5 * s]      # the global bias once, in front of the samples
    ib0 = 0.5 * s
    assert t.ub == [0.5 * s, 0.5 * s] and t.ib[0] == ib0 + 0.5 * (s - 0.125 * ib0)      # item 0 twice, the second time from its new value
    h = 0.5 + 0.5 * (s * 1.0)                           # items are not regularised (positive_reg is what the item gradient reads)
    assert t.W[0][0] == 1.0 + 0.5 * (s * 0.5 - 0.25 * 1.0)
    assert t.H[0][0] == h + 0.5 * (s * 2.0) and t.W[1][0] == 2.0 + 0.5 * (s * h - 0.25 * 2.0)
    # the next batch predicts with the biases
    w0, bias = t.W[0][0], (t.gb[0] + t.ub[0]) + t.ib[1]
    t.apply([0], [1], [2.0], batch_size=8)
    assert t.scalars[1] == 2.0 - (bias + w0 * 0.25) and bias == 0.5 * s + 0.5 * s


@pytest.mark.parametrize("mode", ["adagrad", "rmsprop", "adam"])
def test_first_step_of_the_adaptive_modes_by_hand(mode):
    t = H.Trainer("FUNK_SVD", [[2.0]], [[1.0]], sgd_mode=mode, learning_rate=0.5)
    t.apply([0, 0], [0, 0], [4.0, 4.0], batch_size=1)
    s, g = 2.0, 2.0      # s = rating - 2 * 1; the user gradient is s * H = 2
    if mode == "adagrad":
        step = g / (math.sqrt(g * g) + 1e-8)
    elif mode == "rmsprop":
        step = g / (math.sqrt((1.0 - H.GAMMA) * (g * g)) + 1e-8)
    else:
        step = ((1.0 - H.BETA_1) * g / (1.0 - H.BETA_1)) / (math.sqrt((1.0 - H.BETA_2) * (g * g) / (1.0 - H.BETA_2)) + 1e-8)
    first = H.Trainer("FUNK_SVD", [[2.0]], [[1.0]], sgd_mode=mode, learning_rate=0.5).apply([0], [0], [4.0], batch_size=1)
    assert first.scalars == [s] and first.W[0][0] == 2.0 + 0.5 * step
    assert first.state(0)["USER_factors"][0, 0] != 0.0 and (first.state(1)["USER_factors"][0, 0] != 0.0) == (mode == "adam")
    if mode == "adam":      # the powers move once per batch: two batches, two multiplications
        assert (t.b1p, t.b2p) == (H.BETA_1 * H.BETA_1 * H.BETA_1, H.BETA_2 * H.BETA_2 * H.BETA_2)


def test_the_two_orders_are_the_same_sums():
    rng = np.random.RandomState(3)
    U0, V0 = rng.normal(0, 0.1, (6, 130)), rng.normal(0, 0.1, (9, 130))
    users, items, neg = rng.randint(0, 6, 40), rng.randint(0, 4, 40), rng.randint(4, 9, 40)
    a = H.Trainer("MF_BPR", U0, V0, sgd_mode="adagrad", learning_rate=0.05).apply(users, items, neg, 7).params()
    b = H.Trainer("MF_BPR", U0, V0, sgd_mode="adagrad", learning_rate=0.05, tree=True).apply(users, items, neg, 7).params()
    d = np.abs(a["USER_factors"] - b["USER_factors"]).max()
    assert 0 < d < 1e-12 and np.abs(a["USER_factors"] - U0).max() > 1e-2
    assert H.strided_sum([1.0] * 130) == 130.0 and H.wave_sum(range(64)) == 2016.0


# ---- glibc's rand() and the samplers ------------------------------------------------------------------------------------------------------
def test_glibc_rand_restatement():
    r = H.GlibcRand(1)
    assert [r.rand() for _ in range(5)] == [1804289383, 846930886, 1681692777, 1714636915, 1957747793]      # the documented srand(1) stream
    assert H.GlibcRand(0).rand() == 1804289383      # srand(0) is srand(1)
    assert H.GlibcRand(42).rand() == 71876166


def _profiles():
    rng = np.random.RandomState(0)
    m = (rng.rand(30, 20) < 0.25) * rng.randint(1, 6, size=(30, 20))
    m[0] = 0
    m[1] = 3
    m[2] = 4
    m[2, 19] = 0      # a single possible negative
    return sps.csr_matrix(m.astype(np.float64))


def test_sampler_restatement_properties():
    m = _profiles()
    dense = m.toarray()
    users, items, neg = H.draw("MF_BPR", 11, 0, 20, m, batch_size=8)
    assert users.size == 20 * 32 and not np.any(np.isin(users, [0, 1]))
    assert np.all(dense[users, items] > 0) and np.all(dense[users, neg] == 0) and set(neg[users == 2]) == {19}
    from tests import helpers_slim_bpr as HS      # the triple is SLIM's, index for index
    su, si, sj = HS.draw(11, 0, 1, m)
    assert np.array_equal(users[:31], su) and np.array_equal(items[:31], si) and np.array_equal(neg[:31], sj)
    per = H.per_epoch("FUNK_SVD", m, 8)
    assert per == (m.nnz // 8 + 1) * 8
    u0, i0, r0 = H.draw("FUNK_SVD", 11, 0, 2, m, 8, quota=0.0)
    assert np.array_equal(u0[:32], users[:32]) and np.all(r0 == dense[u0, i0]) and np.all(r0 > 0)      # the same user stream, positives only
    for quota, lo, hi in ((0.3, 0.2, 0.4), (0.999, 0.99, 1.0)):
        u, i, r = H.draw("FUNK_SVD", 11, 0, 4, m, 8, quota=quota)
        assert np.array_equal(u[:2 * per], u0) and np.all(r == dense[u, i])      # a negative has rating 0 and lies outside the profile
        assert lo < np.mean(r > 0) <= hi      # the quota is the share of POSITIVE samples
    e3 = H.draw("FUNK_SVD", 11, 3, 1, m, 8, quota=0.3)
    assert all(np.array_equal(a, b[3 * per:]) for a, b in zip(e3, H.draw("FUNK_SVD", 11, 0, 4, m, 8, quota=0.3)))


def test_reference_sampler_on_the_emulated_stream():
    m = _profiles()
    dense = m.toarray()
    u, i, j = H.reference_samples("MF_BPR", H.GlibcRand(5), 300, m)
    assert not np.any(np.isin(u, [0, 1])) and np.all(dense[u, i] > 0) and np.all(dense[u, j] == 0)
    u, i, r = H.reference_samples("FUNK_SVD", H.GlibcRand(5), 600, m, quota=0.3)
    assert np.all(r == dense[u, i]) and 0.2 < np.mean(r > 0) < 0.4
    first = H.GlibcRand(5).rand() % 30      # the first draw is the first user tried
    assert first in (0, 1) or u[0] == first


# ---- the restatement against the reference's recorded runs --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mf_sgd_tiny.npz"), allow_pickle=False)


def fixture_case(golden, n):
    p = json.loads(str(golden["c%d_params" % n]))
    rates = dict(learning_rate=H.f32(p["learning_rate"]), user_reg=H.f32(p["user_reg"]))
    if p["algorithm"] == "MF_BPR":
        rates.update(positive_reg=H.f32(p["positive_reg"]), negative_reg=H.f32(p["negative_reg"]))
    else:
        rates.update(bias_reg=H.f32(p["bias_reg"]))
    names = H.MEMBERS if p["use_bias"] else H.MEMBERS[:2]
    final = {name: golden["c%d_%s" % (n, name)] for name in names}
    samples = tuple(golden["c%d_%s" % (n, k)] for k in ("users", "items", "third"))
    return p, rates, golden["c%d_U0" % n], golden["c%d_V0" % n], samples, final


def test_fixture_holds_the_cases_and_only_data(golden):
    assert int(golden["n_cases"]) == 12 and int(golden["batch_size"]) == 8 and int(golden["epochs"]) == 3
    seen = set()
    for n in range(12):
        p = json.loads(str(golden["c%d_params" % n]))
        seen.add((p["algorithm"], p["sgd_mode"], p["use_bias"], p["quota"]))
    assert {("MF_BPR", m, False, 0.0) for m in H.MODES} <= seen
    assert {("FUNK_SVD", m, b, q) for m in ("sgd", "adam") for b in (True, False) for q in (0.0, 0.3)} <= seen
    assert tuple(golden["urm_shape"]) == (40, 30)
    assert all(golden[k].dtype.kind in "fiU" for k in golden.files)


@pytest.mark.parametrize("n", range(12))
def test_restatement_reproduces_the_reference(golden, n):
    """R_seq on the list that the glibc restatement predicted, from the recorded initial factors, against the finals the reference's
    compiled epoch left: 1e-12 relative (the tool refuses to write the fixture otherwise)"""
    p, rates, U0, V0, samples, final = fixture_case(golden, n)
    urm = sps.csr_matrix((golden["urm_data"], golden["urm_indices"], golden["urm_indptr"]), shape=tuple(golden["urm_shape"]))
    total = 3 * H.per_epoch(p["algorithm"], urm, 8)
    assert samples[0].size == total
    again = H.reference_samples(p["algorithm"], H.GlibcRand(p["seed"]), total, urm, p["quota"])
    assert all(np.array_equal(a, b) for a, b in zip(samples, again))
    rng = np.random.RandomState(p["seed"])      # np.random.seed(random_seed), then USER, then ITEM
    assert np.array_equal(rng.normal(0.0, 0.1, U0.shape), U0) and np.array_equal(rng.normal(0.0, 0.1, V0.shape), V0)
    got = H.Trainer(p["algorithm"], U0, V0, p["use_bias"], p["sgd_mode"], **rates).apply(*samples, batch_size=8).params()
    for name, ref in final.items():
        err = np.abs(got[name].reshape(ref.shape) - ref).max() / np.abs(ref).max()
        assert err <= 1e-12, (name, err)
    assert np.abs(final["USER_factors"] - U0).max() > 1e-2


# ---- the restated constant -----------------------------------------------------------------------------------------------------------------
def test_the_restated_wave_width_is_the_kernels():
    assert open(os.path.join(ROOT, "ganmf_amd", "csrc", "mf_sgd.hpp")).read().count("constexpr int MF_SGD_WAVE = %d;" % H.WAVE) == 1


# ---- the classes on a helper engine --------------------------------------------------------------------------------------------------------
@pytest.fixture()
def urm():
    return sps.csr_matrix(_profiles(), dtype=np.float32)


def _model(cls_name, urm, **kw):
    from ganmf_amd import MF_SGD
    model = getattr(MF_SGD, cls_name)(urm, **kw)
    model._make_engine = lambda columns: H.HelperEngine(model.n_users, model.n_items, columns)
    return model


def test_bpr_fit_forwards_what_the_reference_forwards(urm):
    model = _model("MatrixFactorization_BPR_Cython", urm)
    model.fit(epochs=2, batch_size=7, num_factors=5, learning_rate=0.01, sgd_mode="adam", user_reg=0.1, item_reg=0.2, bias_reg=0.3,
              positive_reg=0.4, negative_reg=0.5, random_seed=5, use_bias=True, negative_interactions_quota=0.7, init_std_dev=0.2)
    e = model.engine
    # use_bias and the quota are forced; item_reg and bias_reg are not forwarded to a BPR epoch; every rate is a float32 value
    assert e.init_args == dict(algorithm="MF_BPR", use_bias=False, sgd_mode="adam", learning_rate=H.f32(0.01), user_reg=H.f32(0.1),
                               item_reg=0.0, positive_reg=H.f32(0.4), negative_reg=H.f32(0.5), bias_reg=0.0,
                               negative_interactions_quota=0.0, seed=5)
    assert e.init_args["learning_rate"] != 0.01 and model.use_bias is False and model.num_factors == 5
    assert e.t[100].shape == (30, 5) and e.epoch == 2 and e.routes == [(7, 0), (7, 0)] and model.epochs_best == 1
    rng = np.random.RandomState(5)
    assert np.array_equal(e.initial[0], rng.normal(0.0, 0.2, (30, 5))) and np.array_equal(e.initial[1], rng.normal(0.0, 0.2, (20, 5)))
    assert np.array_equal(e.profiles.toarray(), urm.toarray())
    want = H.Trainer("MF_BPR", e.initial[0], e.initial[1], False, "adam", H.f32(0.01), H.f32(0.1), H.f32(0.4), H.f32(0.5)).apply(
        *H.draw("MF_BPR", 5, 0, 2, urm, 7), batch_size=7).params()
    assert model.USER_factors.dtype == np.float64 and np.array_equal(model.USER_factors, want["USER_factors"])
    assert np.array_equal(model.ITEM_factors, want["ITEM_factors"]) and np.array_equal(model.USER_factors_best, model.USER_factors)
    scores = model._compute_item_score(np.arange(4))
    assert np.allclose(scores, want["USER_factors"][:4] @ want["ITEM_factors"].T, rtol=1e-6, atol=1e-9)


def test_funk_fit_with_biases_publishes_two_more_columns(urm):
    model = _model("MatrixFactorization_FunkSVD_Cython", urm)
    model.fit(epochs=1, batch_size=16, num_factors=4, learning_rate=0.02, user_reg=0.1, item_reg=0.2, bias_reg=0.3, positive_reg=0.4,
              negative_reg=0.5, negative_interactions_quota=0.25, random_seed=9)
    e = model.engine
    # positive_reg and negative_reg are never forwarded by FunkSVD's fit(): the item gradient reads a zero
    assert e.init_args == dict(algorithm="FUNK_SVD", use_bias=True, sgd_mode="sgd", learning_rate=H.f32(0.02), user_reg=H.f32(0.1),
                               item_reg=H.f32(0.2), positive_reg=0.0, negative_reg=0.0, bias_reg=H.f32(0.3),
                               negative_interactions_quota=0.25, seed=9)
    assert model.use_bias is True and model.num_factors == 4 and e.t[100].shape == (30, 6) and e.t[101].shape == (20, 6)
    p = e.trainer.params()
    assert np.array_equal(e.t[100][:, 4], p["USER_bias"] + p["GLOBAL_bias"][0]) and np.all(e.t[100][:, 5] == 1.0)
    assert np.all(e.t[101][:, 4] == 1.0) and np.array_equal(e.t[101][:, 5], p["ITEM_bias"])
    assert model.GLOBAL_bias.shape == () and model.GLOBAL_bias == p["GLOBAL_bias"][0] and np.array_equal(model.USER_bias, p["USER_bias"])
    scores = model._compute_item_score(np.arange(30))
    want = p["USER_factors"] @ p["ITEM_factors"].T + p["ITEM_bias"][None, :] + p["GLOBAL_bias"][0] + p["USER_bias"][:, None]
    assert np.allclose(scores, want, rtol=1e-6, atol=1e-9) and np.abs(p["ITEM_bias"]).max() > 0


def test_positive_threshold_filters_the_profiles_of_bpr_only(urm):
    model = _model("MatrixFactorization_BPR_Cython", urm)
    model.fit(epochs=1, positive_threshold_BPR=4, random_seed=1)
    assert np.array_equal(model.engine.profiles.toarray(), (urm.toarray() >= 4).astype(np.float64))
    with pytest.raises(AssertionError, match="URM_train_positive is empty, positive threshold is too high"):
        _model("MatrixFactorization_BPR_Cython", urm).fit(epochs=1, positive_threshold_BPR=6)
    funk = _model("MatrixFactorization_FunkSVD_Cython", urm)
    funk.fit(epochs=1, positive_threshold_BPR=4, random_seed=1)
    assert np.array_equal(funk.engine.profiles.toarray(), urm.toarray()) and funk.engine.profiles.dtype == np.float64


def test_seed_comes_from_numpy_when_none_and_is_used_as_given_otherwise(urm):
    seeds, firsts = [], []
    for _ in range(2):
        np.random.seed(123)
        model = _model("MatrixFactorization_BPR_Cython", urm)
        model.fit(epochs=1)
        seeds.append(model.engine.init_args["seed"])
        firsts.append(model.engine.initial[0])
    assert seeds[0] == seeds[1] and np.array_equal(firsts[0], firsts[1])
    assert np.array_equal(firsts[0], np.random.RandomState(123).normal(0.0, 0.1, (30, 10)))      # the factors are the first draws
    model = _model("MatrixFactorization_BPR_Cython", urm)
    model.fit(epochs=1, random_seed=42)
    assert model.engine.init_args["seed"] == 42


def test_refusals_need_no_device(urm):
    from ganmf_amd import MF_SGD
    asy = MF_SGD.MatrixFactorization_AsySVD_Cython(urm, recompile_cython=True)      # accepted and ignored
    assert asy.RECOMMENDER_NAME == "MatrixFactorization_AsySVD_Cython_Recommender" and asy.algorithm_name == "ASY_SVD"
    with pytest.raises(NotImplementedError, match="last sample drawn in the batch's first phase"):
        asy.fit(epochs=1)
    model = _model("MatrixFactorization_FunkSVD_Cython", urm)
    with pytest.raises(ValueError, match=r"Value for 'sgd_mode' not recognized. Acceptable values are \['sgd', 'adam', 'adagrad', 'rmsprop'\], provided was 'momentum'"):
        model.fit(epochs=1, sgd_mode="momentum")
    with pytest.raises(AssertionError, match="negative_interactions_quota must be a float value >=0 and < 1.0, provided was '1.0'"):
        model.fit(epochs=1, negative_interactions_quota=1.0)
    with pytest.raises(ValueError, match="batch_size must be in"):
        model.fit(epochs=1, batch_size=0)
    with pytest.raises(ValueError, match=r"num_factors \+ 2 \* use_bias must be in \[1, 1024\]"):
        model.fit(epochs=1, num_factors=1023)
    with pytest.raises(ValueError, match=r"num_factors \+ 2 \* use_bias must be in \[1, 1024\]"):
        model.fit(epochs=1, num_factors=0)
    assert model.engine is None
    model.fit(epochs=1, num_factors=1022, batch_size=500, random_seed=1)      # the widest biased model
    with pytest.raises(ValueError, match="epochs_max must be > 0"):
        model.fit(epochs=0)
    with pytest.raises(RuntimeError):
        _model("MatrixFactorization_BPR_Cython", urm).USER_factors
    with pytest.raises(ValueError, match="algorithm_name"):
        MF_SGD._MatrixFactorization_Cython(urm, algorithm_name="SVD++").fit(epochs=1)


class _Evaluator(object):
    """hands out the given MAP values, one per validation, and records the scores and the epoch at that time"""

    def __init__(self, values):
        self.values, self.seen = list(values), []

    def evaluateRecommender(self, model):
        self.seen.append((model.engine.epoch, model._compute_item_score(np.arange(3)), model.USER_factors.copy()))
        return {5: {"MAP": self.values[len(self.seen) - 1]}}, ""


def test_early_stopping_leaves_the_model_of_the_best_validation(urm):
    model = _model("MatrixFactorization_FunkSVD_Cython", urm)
    ev = _Evaluator([0.1, 0.3, 0.2, 0.25])
    model.fit(epochs=20, batch_size=16, num_factors=3, learning_rate=0.05, random_seed=9, validation_every_n=2, stop_on_validation=True,
              validation_metric="MAP", lower_validations_allowed=2, evaluator_object=ev)
    e = model.engine
    assert [s[0] for s in ev.seen] == [2, 4, 6, 8] and e.epoch == 8
    assert (model.epochs_best, model.best_validation_metric) == (4, 0.3) and model.get_early_stopping_final_epochs_dict() == {"epochs": 4}
    # every validation saw its own epoch; fit() leaves the best one's, in the members and in the scores (unlike SLIM_BPR_Cython)
    assert not np.array_equal(ev.seen[1][2], ev.seen[3][2])
    assert np.array_equal(model.USER_factors, ev.seen[1][2]) and np.array_equal(model.USER_factors_best, ev.seen[1][2])
    assert np.array_equal(model._compute_item_score(np.arange(3)), ev.seen[1][1])
    assert not np.array_equal(e.mf_sgd_state()["params"]["USER_factors"], model.USER_factors)      # the training state is epoch 8's


@pytest.mark.parametrize("use_bias", [False, True])
def test_save_and_load_use_the_reference_layout(urm, tmp_path, use_bias):
    model = _model("MatrixFactorization_FunkSVD_Cython", urm)
    model.fit(epochs=2, batch_size=16, num_factors=3, learning_rate=0.05, use_bias=use_bias, random_seed=2)
    model.saveModel(str(tmp_path))
    members = ["ITEM_factors.npy", "USER_factors.npy", "__DataIO_attribute_to_file_name.json", "__DataIO_attribute_to_type_dict.json",
               "_cold_user_mask.npy", "use_bias.json"]
    if use_bias:
        members += ["GLOBAL_bias.npy", "ITEM_bias.npy", "USER_bias.npy"]
    with zipfile.ZipFile(str(tmp_path / "MatrixFactorization_FunkSVD_Cython_Recommender.zip")) as z:
        assert sorted(z.namelist()) == sorted(members)
        assert json.loads(z.read("use_bias.json").decode()) is use_bias
    other = _model("MatrixFactorization_FunkSVD_Cython", urm)
    other.loadModel(str(tmp_path))
    assert other.use_bias is use_bias and other.num_factors == 3
    for name in H.MEMBERS:
        assert np.array_equal(getattr(other, name), getattr(model, name)), name
    assert np.array_equal(other._compute_item_score(np.arange(30)), model._compute_item_score(np.arange(30)))
    if use_bias:      # what FactorModelMixin refuses, and this class alone overrides
        from ganmf_amd.IALS import IALSRecommender
        from tests import helpers_ials as HI
        ials = IALSRecommender(urm)
        ials._make_engine = lambda k: HI.HelperEngine(30, 20, k)
        with pytest.raises(ValueError, match="a saved model with biases is not supported"):
            ials.loadModel(str(tmp_path), file_name="MatrixFactorization_FunkSVD_Cython_Recommender")
