"""SLIM-BPR without a device: the float64 restatement (tests/helpers_slim_bpr.py) against cases worked out by hand, and the
host logic of SLIM_BPR_Cython on a helper engine.  (The level scheduler: tests/test_level_sched_host.py.)"""
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_slim_bpr as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _profiles(rows, n_items):
    m = sps.lil_matrix((len(rows), n_items), dtype=np.float32)
    for u, items in enumerate(rows):
        for s in items:
            m[u, s] = 1.0
    return m.tocsr()


# ---- the update, by hand -----------------------------------------------------------------------------------------------------------------
LR, LI, LJ = 0.05, 0.5, 0.25


def test_sgd_two_samples_by_hand():
    t = H.Trainer(_profiles([[0, 1]], 4), False, "sgd", LR, LI, LJ)
    x, g, upd = t.sample(0, 0, 2)
    assert (x, g, upd) == (0.0, 0.5, 0.5)
    S = t.S()
    want = np.zeros((4, 4))
    want[0, 1] = LR * 0.5                       # s = 1; s = 0 == i is skipped
    want[2, 0] = want[2, 1] = -(LR * 0.5)       # j = 2 is not in the profile: both entries move
    assert np.array_equal(S, want)
    x, g, upd = t.sample(0, 0, 2)
    assert x == (0.0 - want[2, 0]) + (want[0, 1] - want[2, 1])      # ascending s, one running sum
    assert g == 1.0 / (1.0 + math.exp(x)) and upd == g
    S2 = t.S()
    assert S2[0, 1] == want[0, 1] + LR * (g - LI * want[0, 1])
    assert S2[2, 0] == want[2, 0] - LR * (g - LJ * want[2, 0])
    assert S2[2, 1] == want[2, 1] - LR * (g - LJ * want[2, 1])
    assert S2[0, 0] == 0.0 and S2[1].sum() == 0.0 and S2[3].sum() == 0.0


def test_the_s_equals_j_skip_by_hand():
    # an injected j inside the profile: row j skips its own column, row i does not
    t = H.Trainer(_profiles([[0, 1, 2]], 3), False, "sgd", LR, 0.0, 0.0)
    t.sample(0, 0, 2)
    S = t.S()
    assert S[0, 0] == 0.0 and S[0, 1] == S[0, 2] == LR * 0.5
    assert S[2, 2] == 0.0 and S[2, 0] == S[2, 1] == -(LR * 0.5)


@pytest.mark.parametrize("mode", ["adagrad", "rmsprop", "adam"])
def test_first_step_of_the_adaptive_modes_by_hand(mode):
    gamma, b1, b2 = 0.9, 0.8, 0.95
    t = H.Trainer(_profiles([[0, 1], [3]], 5), False, mode, LR, LI, LJ, gamma=gamma, beta_1=b1, beta_2=b2)
    _, g, upd = t.sample(0, 1, 2)
    c0, c1 = t.state()
    assert g == 0.5
    if mode == "adagrad":
        assert c0[1] == c0[2] == 0.25 and upd == 0.5 / (math.sqrt(0.25) + 1e-8)
    elif mode == "rmsprop":
        c = (1.0 - gamma) * 0.25
        assert c0[1] == c0[2] == c and upd == 0.5 / (math.sqrt(c) + 1e-8)
    else:
        m1, m2 = (1.0 - b1) * 0.5, (1.0 - b2) * 0.25
        assert c0[1] == c0[2] == m1 and c1[1] == c1[2] == m2      # the moments of j move too ...
        assert upd == (m1 / (1.0 - b1)) / (math.sqrt(m2 / (1.0 - b2)) + 1e-8)      # ... the step reads those of i only
        assert (t.b1p, t.b2p) == (b1 * b1, b2 * b2)
        # the powers advance once per SAMPLE, whichever items it names: a first touch of item 3 divides by 1 - beta^2
        _, g2, upd2 = t.sample(1, 3, 4)
        assert g2 == 0.5 and upd2 == (m1 / (1.0 - b1 * b1)) / (math.sqrt(m2 / (1.0 - b2 * b2)) + 1e-8)
        assert (t.b1p, t.b2p) == (b1 * b1 * b1, b2 * b2 * b2)
    assert t.S()[1, 0] == LR * upd and t.S()[2, 0] == -(LR * upd) and t.S()[1, 1] == 0.0


def test_symmetric_storage_shares_one_cell_by_hand():
    # (i = 0, s = 1) then (i = 1, s = 0) land in one cell; the dense matrix needs two
    rows = [[0, 1]]
    sym = H.Trainer(_profiles(rows, 4), True, "sgd", LR, 0.0, 0.0)
    den = H.Trainer(_profiles(rows, 4), False, "sgd", LR, 0.0, 0.0)
    for t in (sym, den):
        t.sample(0, 0, 2)
        t.sample(0, 1, 3)
    D, S = den.S(), sym.S()
    assert D[0, 1] == D[1, 0] == LR * 0.5      # two cells, each moved once from zero
    assert np.array_equal(S, S.T)
    x2 = (LR * 0.5 - 0.0) + (0.0 - 0.0)      # second sample: cell(1, 0) is already LR / 2; cell(3, .) is zero
    g2 = 1.0 / (1.0 + math.exp(x2))
    assert S[0, 1] == S[1, 0] == LR * 0.5 + LR * g2
    # and with symmetric storage the negative row reaches the columns of other rows: cell(2, 0) is cell(0, 2)
    assert S[0, 2] == S[2, 0] == -(LR * 0.5)


def test_tree_sum_is_the_same_sum_in_another_order():
    rng = np.random.RandomState(3)
    m = sps.csr_matrix((rng.rand(6, 300) < 0.9).astype(np.float32))
    users, pos, neg = H.draw(5, 0, 6, m)
    a = H.Trainer(m, False, "adagrad", 1e-2, LI, LJ).apply(users, pos, neg).S()
    b = H.Trainer(m, False, "adagrad", 1e-2, LI, LJ, tree_sum=True).apply(users, pos, neg).S()
    assert np.abs(a).max() > 1e-3 and np.allclose(a, b, rtol=0, atol=1e-12)


# ---- get_S and the column top-K, by hand ---------------------------------------------------------------------------------------------------
def test_get_s_and_the_column_topk_by_hand():
    S = np.array([[9.0, 3.0, 3.0, -1.0],
                  [2.0, 9.0, 0.0, 2.0],
                  [0.0, 0.0, 9.0, 0.0],
                  [-2.0, -1.0, -3.0, 9.0]])
    R = H.get_S(S, 2)
    assert R.dtype == np.float32
    # ties go to the smaller id; a row of zeros keeps nothing; in a negative row the zeroed diagonal is the largest value and is dropped
    assert np.array_equal(R, np.array([[0, 3, 3, 0], [2, 0, 0, 2], [0, 0, 0, 0], [0, -1, 0, 0]], dtype=np.float32))
    R1 = H.get_S(S, 1)
    assert np.array_equal(R1, np.array([[0, 3, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float32))
    W = H.w_sparse(S, 2).toarray()      # columns of R: [0 2 0 0] keeps 2 and a zero (dropped); [3 0 0 -1] keeps 3 and a zero: the -1 is cut
    assert np.array_equal(W, np.array([[0, 3, 3, 0], [2, 0, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float32))
    assert np.array_equal(H.w_sparse(S, 9).toarray(), np.where(np.eye(4) > 0, 0, S).astype(np.float32))      # topK > n_items keeps all


# ---- the sampler's restatement -------------------------------------------------------------------------------------------------------------
def test_sampler_restatement_properties():
    n_items = 40
    rows = [[], list(range(n_items)), [7], list(range(n_items - 1)), [1, 5, 9], list(range(0, n_items, 2))]
    m = _profiles(rows, n_items)
    users, pos, neg = H.draw(11, 0, 60, m)
    assert users.size == 60 * (len(rows) + 1)
    assert set(users) == {2, 3, 4, 5}      # never the empty or the full user
    for u, i, j in zip(users, pos, neg):
        assert i in rows[u] and j not in rows[u] and 0 <= j < n_items
    assert set(neg[users == 3]) == {n_items - 1}      # the user with a single possible negative (mostly through the fall-back)
    assert set(pos[users == 4]) == {1, 5, 9}
    again = H.draw(11, 0, 60, m)
    assert all(np.array_equal(a, b) for a, b in zip((users, pos, neg), again))
    other = H.draw(12, 0, 60, m)
    assert not np.array_equal(other[0], users)
    # epochs are addressed, not streamed: epoch 7 alone is the eighth block of epochs 0..7
    e7 = H.draw(11, 7, 1, m)
    assert np.array_equal(e7[2], neg[7 * 7:8 * 7])
    # the user fall-back: one eligible user among 500, further than DRAW_ATTEMPTS draws away for most samples
    lone = _profiles([[]] * 499 + [[3]], 6)
    u2, p2, n2 = H.draw(1, 0, 1, lone)
    assert set(u2) == {499} and set(p2) == {3} and 3 not in set(n2) and len(set(n2)) == 5


def test_generator_words_by_hand():
    # splitmix64's first outputs for the state 0 are published: mix(0) is the first one
    assert H.mix(0) == 0xE220A8397B1DCDAF
    assert H.below(0xFFFFFFFF00000000, 10) == 9 and H.below(0, 10) == 0 and H.below(0x8000000000000000, 7) == 3


# ---- the class on a helper engine ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def urm():
    rng = np.random.RandomState(0)
    m = (rng.rand(30, 20) < 0.25).astype(np.float32) * rng.randint(1, 6, size=(30, 20))
    m[0] = 0
    m[1] = 3
    return sps.csr_matrix(m.astype(np.float32))


def _model(urm, **kw):
    from ganmf_amd.SLIM_BPR import SLIM_BPR_Cython
    model = SLIM_BPR_Cython(urm, **kw)
    model._make_engine = lambda: H.HelperEngine(model.n_users, model.n_items)
    return model


def test_fit_trains_the_given_epochs_and_sets_w_from_the_last_one(urm):
    model = _model(urm)
    model.fit(epochs=3, symmetric=False, random_seed=5, lambda_i=0.1, lambda_j=0.2, learning_rate=0.01, topK=4, sgd_mode="adam",
              gamma=0.9, beta_1=0.8, beta_2=0.95, batch_size=77)
    e = model.engine
    assert e.init_args == dict(symmetric=False, sgd_mode="adam", learning_rate=0.01, lambda_i=0.1, lambda_j=0.2, gamma=0.9, beta_1=0.8,
                               beta_2=0.95, seed=5)
    assert e.epoch == 3 and e.finishes == [(3, 4)] and model.epochs_best == 2
    assert (model.batch_size, model.topK, model.sgd_mode, model.epochs, model.symmetric) == (77, 4, "adam", 3, False)
    assert model.train_with_sparse_weights is False
    # the profiles are URM_train's pattern, the scores are formed from URM_train itself
    assert np.array_equal(e.profiles.toarray(), (urm.toarray() != 0).astype(np.float32))
    assert np.array_equal(e.conf[0].toarray(), urm.toarray())
    t = H.Trainer(urm, False, "adam", 0.01, 0.1, 0.2, 0.9, 0.8, 0.95).apply(*H.draw(5, 0, 3, urm))
    W = model.W_sparse
    assert W.dtype == np.float32 and np.array_equal(W.toarray(), H.w_sparse(t.S(), 4).toarray()) and W.nnz > 0
    # S_incremental: get_S of the last epoch (float64); S_best: its copy at the last epoch when nothing validates
    Sinc = model.S_incremental
    assert Sinc.dtype == np.float64 and np.array_equal(Sinc.toarray().astype(np.float32), H.get_S(t.S(), 4))
    assert np.array_equal(model.S_best.toarray(), Sinc.toarray())
    scores = model._compute_item_score(np.arange(5))
    assert np.allclose(scores, urm[:5].toarray().astype(np.float64) @ W.toarray().astype(np.float64), rtol=1e-5, atol=1e-7)


def test_positive_threshold_filters_the_profiles_only(urm):
    model = _model(urm)
    model.fit(epochs=1, positive_threshold_BPR=4, random_seed=1)
    assert np.array_equal(model.engine.profiles.toarray(), (urm.toarray() >= 4).astype(np.float32))
    assert np.array_equal(model.engine.conf[0].toarray(), urm.toarray())
    with pytest.raises(AssertionError, match="URM_train_positive is empty, positive threshold is too high"):
        _model(urm).fit(epochs=1, positive_threshold_BPR=6)


def test_seed_comes_from_numpy_when_none_and_is_used_as_given_otherwise(urm):
    seeds = []
    for _ in range(2):
        np.random.seed(123)
        model = _model(urm)
        model.fit(epochs=1)
        seeds.append(model.engine.init_args["seed"])
    assert seeds[0] == seeds[1]
    np.random.seed(124)
    model = _model(urm)
    model.fit(epochs=1)
    assert model.engine.init_args["seed"] != seeds[0]
    model = _model(urm)
    model.fit(epochs=1, random_seed=42)
    assert model.engine.init_args["seed"] == 42


def test_refusals_need_no_device(urm):
    from ganmf_amd.SLIM_BPR import SLIM_BPR_Cython
    with pytest.raises(AssertionError, match="free_mem_threshold must be between 0.0 and 1.0, provided was '1.5'"):
        SLIM_BPR_Cython(urm, free_mem_threshold=1.5)
    SLIM_BPR_Cython(urm, recompile_cython=True)      # accepted and ignored
    model = _model(urm)
    with pytest.raises(ValueError, match="train_with_sparse_weights=True"):
        model.fit(epochs=1, train_with_sparse_weights=True)
    with pytest.raises(ValueError, match="TopK not valid. Acceptable values are either False or a positive integer value. Provided value was '0'"):
        model.fit(epochs=1, topK=0)
    with pytest.raises(ValueError, match="SGD_mode not valid. Acceptable values are: 'sgd', 'adagrad', 'rmsprop', 'adam'. Provided value was 'momentum'"):
        model.fit(epochs=1, sgd_mode="momentum")
    with pytest.raises(ValueError, match="epochs_max must be > 0"):
        model.fit(epochs=0)
    assert model.engine is None or isinstance(model.engine, H.HelperEngine)
    big = _model(sps.csr_matrix(np.ones((2, 1500), dtype=np.float32)))
    with pytest.raises(ValueError, match="topK must be at most 1024"):
        big.fit(epochs=1, topK=1200)
    with pytest.raises(RuntimeError):
        _model(urm).W_sparse
    model.fit(epochs=1, train_with_sparse_weights=None, topK=False, random_seed=3)      # None means dense; False keeps every non-zero
    assert model.engine.finishes == [(1, 20)]


class _Evaluator(object):
    """hands out the given MAP values, one per validation, and records what W_sparse was at that time"""

    def __init__(self, values):
        self.values, self.seen = list(values), []

    def evaluateRecommender(self, model):
        self.seen.append((model.engine.epoch, model.W_sparse.toarray()))
        return {5: {"MAP": self.values[len(self.seen) - 1]}}, ""


def test_early_stopping_validates_the_current_s_and_keeps_the_last_epoch(urm):
    model = _model(urm)
    ev = _Evaluator([0.1, 0.3, 0.2, 0.25])
    model.fit(epochs=20, random_seed=9, learning_rate=0.05, topK=5, symmetric=True, sgd_mode="sgd", validation_every_n=2,
              stop_on_validation=True, validation_metric="MAP", lower_validations_allowed=2, evaluator_object=ev)
    e = model.engine
    assert [s[0] for s in ev.seen] == [2, 4, 6, 8] and e.epoch == 8      # two validations in a row without improvement
    assert (model.epochs_best, model.best_validation_metric) == (4, 0.3)
    assert model.get_early_stopping_final_epochs_dict() == {"epochs": 4}
    # every validation saw the W of its own epoch (_prepare_model_for_validation), and fit() leaves the LAST epoch's, not the best one's
    assert e.finishes == [(2, 5), (4, 5), (6, 5), (8, 5), (8, 5)]
    t = H.Trainer(urm, True, "sgd", 0.05, 0.0, 0.0)
    for k, (_, W) in enumerate(ev.seen):
        t.apply(*H.draw(9, 2 * k, 2, urm))
        assert np.array_equal(W, H.w_sparse(t.S(), 5).toarray())
        if k == 1:
            best = H.get_S(t.S(), 5)
    assert np.array_equal(model.W_sparse.toarray(), ev.seen[-1][1])
    assert np.array_equal(model.S_best.toarray().astype(np.float32), best)      # maintained, never read


def test_save_and_load_use_the_reference_layout(urm, tmp_path):
    import zipfile
    model = _model(urm)
    model.fit(epochs=2, random_seed=2, learning_rate=0.05, topK=6)
    model.saveModel(str(tmp_path))
    with zipfile.ZipFile(str(tmp_path / "SLIM_BPR_Recommender.zip")) as z:
        assert sorted(z.namelist()) == ["W_sparse.npz", "__DataIO_attribute_to_file_name.json", "__DataIO_attribute_to_type_dict.json"]
    other = _model(urm)
    other.loadModel(str(tmp_path))
    assert np.array_equal(other.W_sparse.toarray(), model.W_sparse.toarray())
