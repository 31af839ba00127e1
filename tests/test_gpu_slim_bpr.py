"""SLIM-BPR on the device (ganmf_slim_bpr_* on a GANMF_MODEL_ITEMSIM handle) against the float64 restatement of
tests/helpers_slim_bpr.py.

Shapes: 40 users, 70 items (more than one wave) and 400 items; profiles of 1, 2, 63, 64, 65 and n_items - 1 items, one empty and one
full user, and at 400 items one profile of 300 items, longer than the workgroup of 256 threads.

Tolerance of the update tests.  The device and the restatement form the same real sums and products, every operation rounded once
(contraction is off in the kernel); they differ in the ORDER of the profile sum (the device adds 256 strided partial sums by a tree, the
reference one running sum) and by the last place of exp, sqrt and the divisions.  The restatement can sum in either order (tree_sum), and
d = max |S(running sum) - S(tree)| over all of S and the state is the reference's OWN float64 rounding of the profile sum, carried
through the whole list by the true dynamics.  The bound is
    tol = 16 d + 64 * 2^-53 * max |S|
16: the device's remaining differences (exp, sqrt, two divisions: four more roundings per sample, against the L - 1 of a sum over L
items) and the chance that one particular pair of orders differs less than another; 64 ulp of the largest entry: the floor when d
happens to be tiny.  Nothing in it is read from the device."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_slim_bpr as H

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
MODES = ["sgd", "adagrad", "rmsprop", "adam"]
HP = dict(learning_rate=0.02, lambda_i=0.3, lambda_j=0.15, gamma=0.9, beta_1=0.8, beta_2=0.95)


def _urm(n_items, n_users=40, seed=0):
    """the edge profiles of the module docstring among random ones"""
    rng = np.random.RandomState(seed + n_items)
    m = (rng.rand(n_users, n_items) < 0.12).astype(np.float32)
    lengths = [0, n_items, 1, 2, 63, 64, 65, n_items - 1] + ([300] if n_items > 300 else [])
    for u, k in enumerate(lengths):
        m[u] = 0
        m[u, rng.choice(n_items, k, replace=False)] = 1
    return sps.csr_matrix(m)


def _engine(urm, symmetric, mode, seed=0, profiles=None, **hp):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = sps.csr_matrix(urm, dtype=np.float32)
    urm.sort_indices()
    eng = Engine(urm.shape[0], urm.shape[1], 1, 1, 1, model=L.MODEL_ITEMSIM)
    eng.set_confidence(0, urm)
    eng.set_seen(urm)
    kw = dict(HP)
    kw.update(hp)
    eng.slim_bpr_init(symmetric=symmetric, sgd_mode=mode, seed=seed, profiles=profiles, **kw)
    return eng


def _trainer(urm, symmetric, mode, tree_sum=False, **hp):
    kw = dict(HP)
    kw.update(hp)
    return H.Trainer(urm, symmetric, mode, tree_sum=tree_sum, **kw)


def _same_state(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("S", "state0", "state1", "beta_powers"))


def _check_against_restatement(eng, urm, symmetric, mode, samples, label, **hp):
    seq = _trainer(urm, symmetric, mode, **hp).apply(*samples)
    tree = _trainer(urm, symmetric, mode, tree_sum=True, **hp).apply(*samples)
    got = eng.slim_bpr_state()
    worst = 0.0
    for name, a, b in (("S", seq.S(), tree.S()), ("state0", seq.state()[0], tree.state()[0]), ("state1", seq.state()[1], tree.state()[1])):
        d = np.abs(a - b).max()
        tol = 16.0 * d + 64.0 * U53 * np.abs(a).max()
        err = np.abs(got[name] - a).max()
        print("%s %s: max |device - restated| %.3e, d %.3e, tol %.3e, max |value| %.3e" % (label, name, err, d, tol, np.abs(a).max()))
        assert err <= tol, (label, name, err, tol)
        worst = max(worst, err)
    assert np.array_equal(got["beta_powers"], [seq.b1p, seq.b2p])      # formed on the host by the same multiplications
    assert np.abs(seq.S()).max() > 1e-3      # (the list did train something)
    return seq


# ---- the update against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [70, 400])
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_injected_lists_against_the_restatement(mode, symmetric, n_items):
    from ganmf_amd import _lib as L
    urm = _urm(n_items)
    samples = H.draw(17, 0, 4, urm)      # 164 samples: every eligible user several times
    assert {2, 3, 4, 5, 6, 7}.issubset(set(samples[0])) and (n_items < 300 or 8 in set(samples[0]))
    eng = _engine(urm, symmetric, mode)
    levels = eng.slim_bpr_run(*samples, mode=L.SLIM_SEQUENTIAL)
    assert levels == 0
    _check_against_restatement(eng, urm, symmetric, mode, samples, "%s sym=%s n=%d" % (mode, symmetric, n_items))
    if not symmetric:      # the levelled route writes the same bytes
        other = _engine(urm, symmetric, mode)
        levels = other.slim_bpr_run(*samples, mode=L.SLIM_LEVELLED)
        assert 1 < levels < samples[0].size
        assert _same_state(eng.slim_bpr_state(), other.slim_bpr_state())
        other.close()
    eng.close()


def _chains(urm, n):
    """forced chains: one i repeated; one sample's i the next sample's j"""
    lengths = np.diff(urm.indptr)
    u = int(np.flatnonzero(lengths == 65)[0])
    profile = urm.indices[urm.indptr[u]:urm.indptr[u + 1]]
    outside = np.setdiff1d(np.arange(urm.shape[1]), profile)
    rep = (np.full(n, u), np.full(n, profile[0]), outside[np.arange(n) % outside.size])
    # i_t = j_(t+1): user 1 is full, so any item is a positive of theirs; the list is injected, j need not be outside the profile
    ids = np.arange(n + 1) % urm.shape[1]
    link = (np.full(n, 1), ids[:n], ids[1:n + 1])
    return rep, link


@pytest.mark.parametrize("n_items", [70, 400])
@pytest.mark.parametrize("mode", MODES)
def test_levelled_equals_sequential_byte_for_byte(mode, n_items):
    from ganmf_amd import _lib as L
    urm = _urm(n_items)
    rng = np.random.RandomState(5)
    random_list = H.draw(23, 3, 6, urm)
    rep, link = _chains(urm, 30)
    perm = rng.permutation(random_list[0].size + 60)
    mixed = tuple(np.concatenate([a, b, c])[perm] for a, b, c in zip(random_list, rep, link))
    for label, lst, want_levels in (("random", random_list, None), ("repeated i", rep, 30), ("i becomes j", link, 30), ("mixed", mixed, None)):
        a, b = _engine(urm, False, mode), _engine(urm, False, mode)
        assert a.slim_bpr_run(*lst, mode=L.SLIM_SEQUENTIAL) == 0
        levels = b.slim_bpr_run(*lst, mode=L.SLIM_LEVELLED)
        assert levels >= 1 and (want_levels is None or levels == want_levels)
        sa, sb = a.slim_bpr_state(), b.slim_bpr_state()
        assert _same_state(sa, sb), (mode, n_items, label)
        assert np.abs(sa["S"]).max() > 0
        # and a second call continues from the first (the beta powers carry on)
        a.slim_bpr_run(*lst, mode=L.SLIM_AUTO)      # AUTO: levelled for the dense storage
        b.slim_bpr_run(*lst, mode=L.SLIM_SEQUENTIAL)
        assert _same_state(a.slim_bpr_state(), b.slim_bpr_state()), (mode, n_items, label, "second call")
        a.close()
        b.close()


def test_sequential_runs_return_the_same_bytes():
    from ganmf_amd import _lib as L
    urm = _urm(400)
    samples = H.draw(3, 0, 5, urm)
    states = []
    for _ in range(2):
        eng = _engine(urm, True, "adam")
        eng.slim_bpr_run(*samples, mode=L.SLIM_SEQUENTIAL)
        states.append(eng.slim_bpr_state())
        eng.close()
    assert _same_state(*states)


# ---- aliasing and the skips -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sgd", "adam"])
def test_symmetric_aliasing_lands_in_one_cell(mode):
    urm = _urm(70)
    u = int(np.flatnonzero(np.diff(urm.indptr) == 2)[0])
    a, b = (int(s) for s in urm.indices[urm.indptr[u]:urm.indptr[u + 1]])
    outside = [s for s in range(70) if s not in (a, b)][:2]
    samples = (np.array([u, u]), np.array([a, b]), np.array(outside))      # (i = a, s = b) then (i = b, s = a)
    eng = _engine(urm, True, mode)
    eng.slim_bpr_run(*samples)
    S = eng.slim_bpr_state()["S"]
    seq = _check_against_restatement(eng, urm, True, mode, samples, "alias " + mode)
    assert S[a, b] == S[b, a] != 0.0 and np.array_equal(S, S.T)
    one = _trainer(urm, True, mode).apply(*(v[:1] for v in samples)).S()[a, b]
    assert abs(seq.S()[a, b]) > 1.5 * abs(one)      # the cell moved twice
    dense = _engine(urm, False, mode)
    dense.slim_bpr_run(*samples)
    D = dense.slim_bpr_state()["S"]
    assert D[a, b] != 0.0 and D[b, a] != 0.0 and abs(D[a, b]) < abs(S[a, b])      # two cells, each moved once
    dense.close()
    eng.close()


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("mode", ["sgd", "adagrad"])
def test_the_s_equals_i_and_s_equals_j_skips(mode, symmetric):
    """injected lists whose j lies INSIDE the profile: row j skips column j, row i skips column i, the diagonal never moves; with
    symmetric storage cell(i, j) is then written twice in one sample, in the order of s (both orders of i and j)"""
    urm = _urm(70)
    u = int(np.flatnonzero(np.diff(urm.indptr) == 65)[0])
    profile = urm.indices[urm.indptr[u]:urm.indptr[u + 1]]
    outside = np.setdiff1d(np.arange(70), profile)
    samples = (np.array([u, u, u, 1, u]), np.array([profile[3], profile[9], profile[0], 5, profile[20]]),
               np.array([profile[8], profile[2], outside[0], 6, profile[64]]))      # j inside (i < j and i > j), outside, full user, inside
    eng = _engine(urm, symmetric, mode)
    eng.slim_bpr_run(*samples)
    _check_against_restatement(eng, urm, symmetric, mode, samples, "skips %s sym=%s" % (mode, symmetric))
    S = eng.slim_bpr_state()["S"]
    assert np.all(np.diag(S) == 0.0)
    eng.close()


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [70, 400])
def test_sampler_equals_its_restatement_and_respects_the_profiles(n_items):
    urm = _urm(n_items)
    eng = _engine(urm, True, "sgd", seed=99)
    users, pos, neg = eng.slim_bpr_draw(0, 12)
    assert users.size == 12 * 41 and users.dtype == np.int32
    want = H.draw(99, 0, 12, urm)
    assert all(np.array_equal(a, b) for a, b in zip((users, pos, neg), want))
    dense = urm.toarray() > 0
    assert not np.any(np.isin(users, [0, 1]))      # never the empty or the full user
    assert np.all(dense[users, pos]) and not np.any(dense[users, neg])
    single = int(np.flatnonzero(np.diff(urm.indptr) == n_items - 1)[0])
    assert np.any(users == single) and set(neg[users == single]) == set(np.flatnonzero(~dense[single]))
    assert set(users) == set(range(2, 40))
    # addressed by epoch: a later call for epoch 7 alone returns epoch 7 of the long call, and nothing of the state moved
    e7 = eng.slim_bpr_draw(7, 1)
    assert all(np.array_equal(a, b[7 * 41:8 * 41]) for a, b in zip(e7, (users, pos, neg)))
    again = eng.slim_bpr_draw(0, 12)
    assert all(np.array_equal(a, b) for a, b in zip(again, (users, pos, neg)))
    state = eng.slim_bpr_state()
    assert state["epoch"] == 0 and not state["S"].any()
    other = _engine(urm, True, "sgd", seed=100)
    assert not np.array_equal(other.slim_bpr_draw(0, 12)[0], users)
    same = _engine(urm, True, "sgd", seed=99)
    assert np.array_equal(same.slim_bpr_draw(0, 12)[2], neg)
    assert eng.slim_bpr_draw(5, 0)[0].size == 0
    for e in (eng, other, same):
        e.close()


def test_sampler_user_fallback_and_given_profiles():
    """one eligible user among 500 (further than DRAW_ATTEMPTS draws away for most samples), and profiles that are not side 0"""
    rows = np.zeros((500, 6), dtype=np.float32)
    rows[499, 3] = 1
    rows[7] = 1
    profiles = sps.csr_matrix(rows)
    urm = sps.csr_matrix(np.ones((500, 6), dtype=np.float32))      # side 0: every user full
    eng = _engine(urm, False, "sgd", seed=4, profiles=profiles)
    got = eng.slim_bpr_draw(2, 1)
    assert all(np.array_equal(a, b) for a, b in zip(got, H.draw(4, 2, 1, profiles)))
    assert set(got[0]) == {499} and set(got[1]) == {3} and set(got[2]) == {0, 1, 2, 4, 5}
    eng.close()


def test_epochs_is_draw_followed_by_run():
    from ganmf_amd import _lib as L
    urm = _urm(70)
    for symmetric, route in ((False, L.SLIM_AUTO), (False, L.SLIM_SEQUENTIAL), (True, L.SLIM_AUTO)):
        a, b = _engine(urm, symmetric, "adam", seed=8), _engine(urm, symmetric, "adam", seed=8)
        levels = a.slim_bpr_epochs(3, mode=route)
        assert (levels > 1) == (not symmetric and route == L.SLIM_AUTO)
        a.slim_bpr_epochs(2, mode=route)
        b.slim_bpr_run(*b.slim_bpr_draw(0, 5), mode=L.SLIM_SEQUENTIAL)
        sa, sb = a.slim_bpr_state(), b.slim_bpr_state()
        assert _same_state(sa, sb) and sa["epoch"] == 5 and sb["epoch"] == 0 and np.abs(sa["S"]).max() > 0
        a.close()
        b.close()


def test_nobody_to_sample_is_an_error_not_a_hang():
    from ganmf_amd import _lib as L
    rows = np.zeros((5, 9), dtype=np.float32)
    rows[1] = rows[3] = 1
    with pytest.raises(L.GanmfError, match=r"\(-1\).*neither empty nor full"):
        _engine(sps.csr_matrix(rows), True, "sgd")


# ---- finish -----------------------------------------------------------------------------------------------------------------------------------
def _same_bytes(a, b):
    a, b = sps.csr_matrix(a), sps.csr_matrix(b)
    a.sort_indices()
    b.sort_indices()
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and \
        a.data.dtype == b.data.dtype == np.float32 and a.data.tobytes() == b.data.tobytes()


@pytest.mark.parametrize("n_items", [70, 400])
@pytest.mark.parametrize("symmetric", [False, True])
def test_finish_against_the_restatement_on_the_device_s_own_s(symmetric, n_items):
    """both top-K passes move values only (one rounding to float32 between them): checked EXACTLY against helpers_slim_bpr.w_sparse
    applied to the S read back from the device"""
    urm = _urm(n_items)
    # full of ties: the first sgd epoch without regularisation moves every touched cell by the same +- lr / 2 ... lr g
    tie = _engine(urm, symmetric, "sgd", seed=1, lambda_i=0.0, lambda_j=0.0, learning_rate=0.25)
    tie.slim_bpr_epochs(1)
    S = tie.slim_bpr_state()["S"]
    vals, counts = np.unique(S[S != 0], return_counts=True)
    assert counts.max() >= 20      # (ties there are)
    for topk in (1, 5, 64, n_items - 1, n_items, n_items + 50):
        nnz = tie.slim_bpr_finish(topk)
        W = tie.item_similarity()
        want = H.w_sparse(S, topk)
        assert W.nnz == nnz == want.nnz and _same_bytes(W, want), (topk, W.nnz, want.nnz)
        assert np.all(W.diagonal() == 0)
    assert tie.slim_bpr_state()["S"].tobytes() == S.tobytes()      # S survives (its diagonal was zero already)
    tie.close()
    # tie-free: several adam epochs with regularisation
    eng = _engine(urm, symmetric, "adam", seed=2)
    eng.slim_bpr_epochs(6)
    S = eng.slim_bpr_state()["S"]
    for topk in (3, 40):
        nnz = eng.slim_bpr_finish(topk)
        W = eng.item_similarity()
        assert W.nnz == nnz and _same_bytes(W, H.w_sparse(S, topk))
        assert np.diff(sps.csc_matrix(W).indptr).max() <= topk
    if not symmetric:      # the orientation: W[a, b] = S[a, b], not its transpose
        Wd = W.toarray()
        a, b = np.nonzero(Wd)
        assert np.array_equal(Wd[a, b], S[a, b].astype(np.float32)) and not np.allclose(S, S.T)
    # training continues after finish: the same bytes as an uninterrupted run
    eng.slim_bpr_epochs(2)
    straight = _engine(urm, symmetric, "adam", seed=2)
    straight.slim_bpr_epochs(8)
    assert _same_state(eng.slim_bpr_state(), straight.slim_bpr_state())
    # and the scores are URM . W
    eng.slim_bpr_finish(40)
    W = eng.item_similarity()
    ids = np.arange(40)
    ref = urm.toarray().astype(np.float64) @ W.toarray().astype(np.float64)
    got = eng.scores(ids)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    eng.close()
    straight.close()


# ---- the class ---------------------------------------------------------------------------------------------------------------------------------
def test_two_fits_give_identical_bytes_and_the_class_recommends_and_evaluates():
    from SLIM_BPR.Cython.SLIM_BPR_Cython import SLIM_BPR_Cython
    from ganmf_amd import _lib as L
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    rng = np.random.RandomState(1)
    ratings = sps.csr_matrix(_urm(70).multiply(rng.randint(1, 6, size=(40, 70))).astype(np.float32))
    test = sps.csr_matrix(((rng.rand(40, 70) < 0.1) & (ratings.toarray() == 0)).astype(np.float32))
    Ws = []
    for k, route in enumerate((L.SLIM_AUTO, L.SLIM_AUTO, L.SLIM_SEQUENTIAL)):
        model = SLIM_BPR_Cython(ratings)
        model.train_route = route
        model.fit(epochs=6, symmetric=False, random_seed=31, learning_rate=0.05, lambda_i=0.01, lambda_j=0.001, topK=10, sgd_mode="adagrad",
                  positive_threshold_BPR=2, validation_every_n=3, validation_metric="MAP", evaluator_object=EvaluatorHoldoutFast(test, [5]))
        Ws.append(model.W_sparse)
        if k < 2:
            model.engine.close()
    assert _same_bytes(Ws[0], Ws[1]) and _same_bytes(Ws[0], Ws[2]) and Ws[0].nnz > 0
    assert model.epochs_best in (3, 6) and model.best_validation_metric is not None
    # the restatement of the whole fit: the profiles are the ratings >= 2, the scores use the ratings themselves
    positive = sps.csr_matrix((ratings.toarray() >= 2).astype(np.float32))
    seq = H.Trainer(positive, False, "adagrad", 0.05, 0.01, 0.001).apply(*H.draw(31, 0, 6, positive))
    S = model.engine.slim_bpr_state()["S"]
    # (the plumbing of a whole fit, not the arithmetic: that has its bound in test_injected_lists_against_the_restatement)
    assert np.allclose(S, seq.S(), rtol=0, atol=1e-9 * np.abs(S).max()) and np.abs(S).max() > 0.01
    assert _same_bytes(Ws[0], H.w_sparse(S, 10))
    assert np.array_equal(model.S_incremental.toarray().astype(np.float32), H.get_S(S, 10))
    recs = model.recommend(np.arange(40), cutoff=5)
    scores = ratings.toarray().astype(np.float64) @ Ws[0].toarray().astype(np.float64)
    scores[ratings.toarray() > 0] = -np.inf
    for u in range(9, 40):      # (the random profiles: at least five unseen items)
        assert len(recs[u]) == 5 and not set(recs[u]) & set(ratings[u].indices)
        assert np.allclose(np.sort(scores[u])[::-1][:5], scores[u, recs[u]], rtol=1e-4, atol=1e-6)
    results, _ = EvaluatorHoldoutFast(test, [5]).evaluateRecommender(model)
    assert 0.0 <= results[5]["MAP"] <= 1.0
    if model.epochs_best == 6:      # the model left by fit() is the last epoch's: its validation was the best one
        assert results[5]["MAP"] == model.best_validation_metric
    model.engine.close()


# ---- error paths -------------------------------------------------------------------------------------------------------------------------------
def test_error_paths_of_every_entry():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = _urm(70)
    urm.sort_indices()
    eng = Engine(40, 70, 1, 1, 1, model=L.MODEL_ITEMSIM)
    # one good sample: user 3 has two items (a user with one item moves only the negative row)
    ok = (np.array([3]), np.array([int(urm[3].indices[0])]), np.array([int(np.setdiff1d(np.arange(70), urm[3].indices)[0])]))
    # nothing before init
    for call in (lambda: eng.slim_bpr_draw(0, 1), lambda: eng.slim_bpr_run(*ok), lambda: eng.slim_bpr_epochs(1), lambda: eng.slim_bpr_finish(5),
                 lambda: eng.slim_bpr_state()):
        with pytest.raises(L.GanmfError, match="ganmf_slim_bpr_init has not been called"):
            call()
    with pytest.raises(L.GanmfError, match="side 0"):
        eng.slim_bpr_init()      # no profiles given and no side 0 uploaded
    eng.set_confidence(0, urm)
    with pytest.raises(ValueError, match="SGD_mode not valid"):
        eng.slim_bpr_init(sgd_mode="momentum")
    with pytest.raises(L.GanmfError, match="unknown sgd mode"):
        L.check(eng.lib.ganmf_slim_bpr_init(eng.h, 1, 9, 0.1, 0.0, 0.0, 0.9, 0.9, 0.99, 0, None, None), "ganmf_slim_bpr_init")
    with pytest.raises(L.GanmfError, match="must be finite"):
        eng.slim_bpr_init(learning_rate=float("nan"))
    with pytest.raises(L.GanmfError, match=r"beta_1 and beta_2 must be in \[0, 1\)"):
        eng.slim_bpr_init(sgd_mode="adam", beta_1=1.0)
    unsorted = sps.csr_matrix(urm, copy=True)
    unsorted.indices[urm.indptr[4]:urm.indptr[4] + 2] = unsorted.indices[urm.indptr[4]:urm.indptr[4] + 2][::-1].copy()
    with pytest.raises(L.GanmfError, match="not sorted"):
        L.check(eng.lib.ganmf_slim_bpr_init(eng.h, 1, 0, 0.1, 0.0, 0.0, 0.9, 0.9, 0.99, 0,
                                            np.ascontiguousarray(unsorted.indptr, dtype=np.int64).ctypes.data_as(L.C.POINTER(L.C.c_int64)),
                                            np.ascontiguousarray(unsorted.indices, dtype=np.int32).ctypes.data_as(L.C.POINTER(L.C.c_int32))),
                "ganmf_slim_bpr_init")
    with pytest.raises(ValueError, match="profiles must be 40 x 70"):
        eng.slim_bpr_init(profiles=sps.csr_matrix((40, 71), dtype=np.float32))
    # still no state after the refusals; then a symmetric one
    with pytest.raises(L.GanmfError, match="has not been called"):
        eng.slim_bpr_state()
    eng.slim_bpr_init(symmetric=True, sgd_mode="sgd", learning_rate=0.1)
    with pytest.raises(L.GanmfError, match="levelled route needs symmetric = 0"):
        eng.slim_bpr_run(*ok, mode=L.SLIM_LEVELLED)
    with pytest.raises(L.GanmfError, match="levelled route needs symmetric = 0"):
        eng.slim_bpr_epochs(1, mode=L.SLIM_LEVELLED)
    with pytest.raises(L.GanmfError, match="unknown route"):
        eng.slim_bpr_run(*ok, mode=7)
    for bad, what in (((np.array([40]), ok[1], ok[2]), "names user 40 of 40"), ((ok[0], np.array([70]), ok[2]), "names item"),
                      ((ok[0], ok[1], np.array([-1])), "names item"), ((ok[0], ok[1], ok[1]), "same positive and negative")):
        with pytest.raises(L.GanmfError, match=what):
            eng.slim_bpr_run(*bad)
    with pytest.raises(L.GanmfError, match="must be >= 0"):
        eng.slim_bpr_draw(-1, 1)
    with pytest.raises(L.GanmfError, match="must be >= 0"):
        eng.slim_bpr_epochs(-1)
    with pytest.raises(L.GanmfError, match="topk 0 must be >= 1"):
        eng.slim_bpr_finish(0)
    assert not eng.slim_bpr_state()["S"].any()      # nothing was enqueued by a refused call
    assert eng.slim_bpr_run(np.zeros(0), np.zeros(0), np.zeros(0)) == 0      # an empty list is allowed
    eng.slim_bpr_run(*ok)
    assert eng.slim_bpr_finish(5) > 0
    eng.close()
    mf = Engine(40, 70, 2, 1, 1, model=L.MODEL_MF)
    with pytest.raises(L.GanmfError, match="ITEMSIM"):
        mf.slim_bpr_init(profiles=urm)
    mf.close()
    wide = Engine(3, 1500, 1, 1, 1, model=L.MODEL_ITEMSIM)
    wide.slim_bpr_init(profiles=sps.csr_matrix(np.eye(3, 1500, dtype=np.float32)))
    with pytest.raises(L.GanmfError, match="GANMF_ITEMKNN_MAX_TOPK"):
        wide.slim_bpr_finish(1200)
    assert wide.slim_bpr_finish(1024) == 0      # S is zero
    wide.close()


def test_a_failed_allocation_names_the_bytes_and_leaves_the_handle_usable():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    n = 400000      # S would need 8 n^2 = 1.28e12 bytes
    eng = Engine(3, n, 1, 1, 1, model=L.MODEL_ITEMSIM)
    profiles = sps.csr_matrix((np.ones(3, dtype=np.float32), (np.arange(3), np.arange(3))), shape=(3, n))
    with pytest.raises(MemoryError, match=r"out of memory: S .* needs %d bytes" % (8 * n * n)):
        eng.slim_bpr_init(symmetric=False, profiles=profiles)
    with pytest.raises(L.GanmfError, match="has not been called"):
        eng.slim_bpr_epochs(1)
    W = sps.csr_matrix((np.ones(2, dtype=np.float32), ([0, 1], [1, 0])), shape=(n, n))
    eng.set_item_similarity(W)      # the handle still works
    assert eng.item_similarity().nnz == 2
    eng.close()


# ---- the reference's logged ML-1M trials --------------------------------------------------------------------------------------------------
def _trial_doc():
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slim_bpr_trial_logs_ml1m.json")))


_TRIALS = _trial_doc()["trials"]


@pytest.fixture(scope="module")
def ml1m(golden_dir):
    import os
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    doc = _trial_doc()
    train = sps.load_npz(os.path.join(golden_dir, doc["train"])).tocsr()
    valid = sps.load_npz(os.path.join(golden_dir, doc["validation"])).tocsr()
    return train, EvaluatorHoldoutFast(valid, [doc["at"]])


def test_trial_fixture_covers_both_storages_and_the_searched_modes():
    doc = _trial_doc()
    assert {t["params"]["symmetric"] for t in _TRIALS} == {True, False}
    assert {t["params"]["sgd_mode"] for t in _TRIALS} == {"sgd", "adagrad", "adam"}
    for t in _TRIALS:
        assert t["params"]["epochs"] <= 100 and len(t["seeds"]) >= 5 and t["seeds"][0] == 1 and len(t["values"]) == len(t["seeds"])
        assert abs(np.mean(t["values"]) - t["mean"]) < 1e-12 and abs(np.std(t["values"], ddof=1) - t["std"]) < 1e-12
        assert t["bound"] == 3.0 * t["std"]      # three of OUR measured standard deviations, as recorded


@pytest.mark.parametrize("n", range(len(_TRIALS)), ids=lambda n: "%s-sym%s-%d" % (_TRIALS[n]["params"]["sgd_mode"], _TRIALS[n]["params"]["symmetric"], n))
def test_logged_trial_replayed_on_the_device(ml1m, n):
    """MAP@5 on the validation split of one logged ML-1M trial, trained on train_small with seed 1 for the logged epochs + 25 (the
    reference logs the epoch of its best validation and evaluates the model 25 epochs later): |MAP(seed 1) - logged| <= 3 standard
    deviations of MAP over five seeds of ours (the fixture's `bound`, measured by tools/slim_bpr_bench.py --trials).  The reference's
    own runs are unseeded, so the logged value is one draw of its distribution; profiles/slim_bpr_fit.md holds the table."""
    from ganmf_amd.SLIM_BPR import SLIM_BPR_Cython
    train, ev = ml1m
    doc = _trial_doc()
    t = _TRIALS[n]
    p = dict(t["params"])
    p["epochs"] += doc["epochs_after_best"]
    model = SLIM_BPR_Cython(train.copy())
    model.fit(random_seed=t["seeds"][0], **p)
    got = ev.evaluateRecommender(model)[0][doc["at"]][doc["metric"]]
    model.engine.close()
    print("slim-bpr trial %s symmetric %s topK %d epochs %d + %d: seed %d gives %.7f (measured %.7f), logged %.7f, mean %.7f std %.2e; "
          "|seed - logged| %.2e, bound %.2e" % (p["sgd_mode"], p["symmetric"], p["topK"], t["params"]["epochs"], doc["epochs_after_best"],
                                                 t["seeds"][0], got, t["values"][0], t["logged"], t["mean"], t["std"],
                                                 abs(got - t["logged"]), t["bound"]))
    assert abs(got - t["logged"]) <= t["bound"]
