"""Item-KNN on the device (ganmf_itemknn_fit / ganmf_set_item_similarity / the sparse score source of a GANMF_MODEL_ITEMSIM handle)
against the float64 restatement of tests/helpers_itemknn.py.

W is checked for VALIDITY, with no case left out (_check_sparse): a column holds min(topK, number of non-zero
similarities) entries, no duplicate, no self entry; every stored (j, v) has |v - sim64[j, i]| <= tau; the values sorted descending
equal the helper's top values within tau.  tau is derived: on integer-valued matrices every dot product w is an integer below 2^24,
exact in fp32 (asserted exactly on a RAW fit); the value is then at most eight fp32 roundings away, tau = 16 * 2^-24 * |v|.  On BM25 /
TF-IDF data (all terms non-negative) the FMA chain of len_i terms adds len_i roundings: tau = (len_i + 16) * 2^-24 * |v|.
Scores: |device - float64 URM . W| <= (L + 2) * 2^-24 * score, L the number of terms of that score (non-negative operands)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_itemknn as H

pytestmark = pytest.mark.gpu

EPS = H.EPS32


# ---- matrices and engines -------------------------------------------------------------------------------------------------------
def _ratings(n_users, n_items, density, seed, per_user=None):
    rng = np.random.RandomState(seed)
    if per_user is not None:      # exactly `per_user` entries per user
        cols = np.array([rng.permutation(n_items)[:per_user] for _ in range(n_users)]).ravel()
        rows = np.repeat(np.arange(n_users), per_user)
        vals = rng.randint(1, 6, len(rows)).astype(np.float32)
        return sps.csr_matrix((vals, (rows, cols)), shape=(n_users, n_items))
    m = sps.random(n_users, n_items, density=density, format="csr", random_state=rng, dtype=np.float32)
    m.data = rng.randint(1, 6, m.nnz).astype(np.float32)
    return m


def _edge_matrix():
    """70 x 50 at density 0.2 with an empty item column (3), an empty user row (5), a one-entry column (8), and a column (13) with
    fewer non-zero similarities than topK = 5: its only two users rated nothing else but items 14 and 15"""
    m = _ratings(70, 50, 0.2, 7).tolil()
    m[:, 3] = 0
    m[5, :] = 0
    m[:, 8] = 0
    m[11, 8] = 4
    m[:, 13] = 0
    m[20, :] = 0
    m[21, :] = 0
    m[20, 13], m[20, 14] = 2, 3
    m[21, 13], m[21, 15] = 5, 1
    m = sps.csr_matrix(m, dtype=np.float32)
    m.eliminate_zeros()
    return m


def _engine(urm, binarise=False):
    """a GANMF_MODEL_ITEMSIM engine holding `urm` in both orientations (side 1 as ones when the similarity binarises)"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = sps.csr_matrix(urm, dtype=np.float32)
    urm.sort_indices()
    eng = Engine(urm.shape[0], urm.shape[1], 1, 1, 1, model=L.MODEL_ITEMSIM)
    eng.set_confidence(0, urm)
    seen = urm.copy()
    if binarise:
        seen.data[:] = 1.0
    t = seen.tocsc()
    t.sort_indices()
    eng.set_confidence(1, sps.csr_matrix((t.data, t.indices, t.indptr), shape=(urm.shape[1], urm.shape[0])))
    eng.set_seen(urm)
    return eng


def _sparse_similarity(urm, kind, shrink, p0, p1, den_a, den_b):
    """helpers_itemknn.similarity_dense at the non-zero dot products only (CSC float64, no diagonal): the form that also fits a
    33 000-item catalogue.  Values at zero dot products are zero under every kind."""
    X = sps.csc_matrix(urm, dtype=np.float64)
    w = sps.csc_matrix(X.T.dot(X))
    w.setdiag(0.0)
    w.eliminate_zeros()
    w.sort_indices()
    j = w.indices
    i = np.repeat(np.arange(w.shape[1]), np.diff(w.indptr))
    s = float(shrink) + 1e-6
    v = w.data
    if kind == H.PRODUCT:
        v = v / (den_a[i] * den_b[j] + s)
    elif kind == H.TANIMOTO:
        v = v / (den_a[i] + den_a[j] - v + s)
    elif kind == H.DICE:
        v = v / (den_a[i] + den_a[j] + s)
    elif kind == H.TVERSKY:
        v = v / (v + (den_a[i] - v) * p0 + (den_a[j] - v) * p1 + s)
    elif kind == H.SHRINK_ONLY:
        v = v / float(shrink)
    return sps.csc_matrix((v, j, w.indptr), shape=w.shape)


def _check_sparse(W_dev, sim, topk, tau_scale):
    """The validity check of a device W against the float64 similarities `sim` (CSC, the non-zero ones): per column the four
    conditions of the module's docstring, tau_scale[i] * |v| being column i's bound.  Returns the largest error / bound seen."""
    W = sps.csc_matrix(W_dev)
    W.sort_indices()
    n = sim.shape[0]
    k = min(topk, n)
    worst = 0.0
    for i in range(n):
        idx = W.indices[W.indptr[i]:W.indptr[i + 1]]
        val = W.data[W.indptr[i]:W.indptr[i + 1]].astype(np.float64)
        ref_j = sim.indices[sim.indptr[i]:sim.indptr[i + 1]]
        ref_v = sim.data[sim.indptr[i]:sim.indptr[i + 1]]
        keep = np.lexsort((ref_j, -ref_v))[:k]
        assert len(idx) == len(keep), "column %d holds %d entries, %d expected" % (i, len(idx), len(keep))
        if len(idx) == 0:
            continue
        assert len(np.unique(idx)) == len(idx) and i not in idx, "column %d: duplicate or self entry" % i
        pos = np.searchsorted(ref_j, idx)
        assert np.all(pos < len(ref_j)) and np.all(ref_j[np.minimum(pos, len(ref_j) - 1)] == idx), \
            "column %d keeps a neighbour whose similarity is zero" % i
        own = ref_v[pos]
        err = np.abs(val - own)
        assert np.all(err <= tau_scale[i] * np.abs(own)), "column %d: a stored value is off by %g (bound %g)" % (
            i, err.max(), (tau_scale[i] * np.abs(own))[err.argmax()])
        top = ref_v[keep]
        err_sorted = np.abs(np.sort(val)[::-1] - top)
        assert np.all(err_sorted <= tau_scale[i] * np.abs(top)), "column %d: the kept values are not the largest ones" % i
        worst = max(worst, float((err / (tau_scale[i] * np.abs(own))).max()))
    return worst


KIND_SETTINGS = [      # (similarity, normalize, shrink, extra): every kind the device has
    ("cosine", True, 10, {}), ("asymmetric", True, 0, dict(asymmetric_alpha=0.3)), ("jaccard", True, 3, {}), ("dice", True, 0, {}),
    ("tversky", True, 2, dict(tversky_alpha=0.7, tversky_beta=1.5)), ("cosine", False, 5, {}), ("cosine", False, 0, {})]


def _fit_and_check(urm, similarity, normalize, shrink, extra, topk, weighted=False):
    kind, X, p0, p1, den_a, den_b = H.host_plan(urm, similarity, normalize, shrink, **extra) if urm.shape[1] <= 2000 else \
        _plan_sparse(urm, similarity, normalize, shrink, **extra)
    binarise = kind in (H.TANIMOTO, H.DICE, H.TVERSKY)
    eng = _engine(urm, binarise)
    seen = sps.csr_matrix(urm, dtype=np.float32, copy=True)
    if binarise:
        seen.data[:] = 1.0
    a32 = None if den_a is None else den_a.astype(np.float32)
    b32 = None if den_b is None else den_b.astype(np.float32)
    nnz = eng.itemknn_fit(kind, topk, shrink=shrink, p0=p0, p1=p1, den_a=a32, den_b=b32)
    W = eng.item_similarity()
    assert W.nnz == nnz and W.dtype == np.float32
    # the helper sees what the device sees: float32 data, float32 denominators, float32 coefficients
    sim = _sparse_similarity(seen, kind, np.float32(shrink), np.float32(p0), np.float32(p1),
                             None if a32 is None else a32.astype(np.float64), None if b32 is None else b32.astype(np.float64))
    lens = np.diff(sps.csc_matrix(seen).indptr)
    tau = (lens + 16.0) * EPS if weighted else np.full(urm.shape[1], 16.0 * EPS)
    worst = _check_sparse(W, sim, topk, tau)
    print("itemknn %s normalize=%s shrink=%s %s topK=%d: %d x %d, nnz %d, worst error / tau %.3f" % (
        similarity, normalize, shrink, extra, topk, urm.shape[0], urm.shape[1], nnz, worst))
    return eng, W, sim


def _plan_sparse(urm, similarity, normalize, shrink, **extra):
    """host_plan without the dense copy (wide catalogues): cosine / raw only"""
    assert similarity == "cosine"
    sq = np.asarray(sps.csc_matrix(urm, dtype=np.float64).power(2).sum(axis=0)).ravel()
    if normalize:
        return H.PRODUCT, None, 1.0, 1.0, np.sqrt(sq), np.sqrt(sq)
    return (H.SHRINK_ONLY if shrink != 0 else H.RAW), None, 1.0, 1.0, None, None


# ---- W against the helper ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topk", [1, 5, 49, 50, 1000])
@pytest.mark.parametrize("setting", KIND_SETTINGS, ids=lambda s: "%s-%s-%s" % s[:3])
def test_fit_every_kind_and_topk(setting, topk):
    eng, _, _ = _fit_and_check(_ratings(70, 50, 0.2, 1), *setting, topk=topk)
    eng.close()


@pytest.mark.parametrize("setting", KIND_SETTINGS, ids=lambda s: "%s-%s-%s" % s[:3])
def test_fit_structural_edges(setting):
    urm = _edge_matrix()
    for topk in (1, 5, 50):
        eng, W, _ = _fit_and_check(urm, *setting, topk=topk)
        W = sps.csc_matrix(W)
        assert W[:, 3].nnz == 0 and W[3, :].nnz == 0      # the empty item: no neighbours, nobody's neighbour
        assert W[:, 13].nnz == min(topk, 2) and set(W[:, 13].indices) <= {14, 15}
        eng.close()


def test_raw_dot_products_are_exact_integers():
    urm = _ratings(70, 50, 0.2, 1)
    eng = _engine(urm)
    eng.itemknn_fit(H.RAW, 50)
    W = np.asarray(eng.item_similarity().todense(), dtype=np.float64)
    X = H.dense64(urm)
    w = X.T.dot(X)
    np.fill_diagonal(w, 0.0)
    assert w.max() < 2 ** 24
    np.testing.assert_array_equal(W, w)      # all 49 neighbours kept: the whole (symmetric) matrix, exactly
    eng.close()


@pytest.mark.parametrize("n_items", [1, 2, 257])
def test_fit_small_and_multi_block_catalogues(n_items):
    urm = _ratings(90, n_items, 0.3, n_items)
    for setting in (KIND_SETTINGS[0], KIND_SETTINGS[2], KIND_SETTINGS[6]):
        eng, W, _ = _fit_and_check(urm, *setting, topk=5)
        if n_items == 1:
            assert W.nnz == 0
        eng.close()


def test_fit_topk_1000_of_1100_items():
    eng, W, _ = _fit_and_check(_ratings(60, 1100, 0.3, 5), "cosine", True, 4, {}, topk=1000)
    assert np.diff(sps.csc_matrix(W).indptr).max() == 1000
    eng.close()


def test_fit_more_users_than_one_lds_slab():
    urm = _ratings(40000, 130, None, 9, per_user=3)
    for setting in (KIND_SETTINGS[0], KIND_SETTINGS[4], KIND_SETTINGS[6]):
        eng, _, _ = _fit_and_check(urm, *setting, topk=20)
        eng.close()


def test_fit_row_above_the_lds_cap():
    urm = _ratings(300, 33000, 0.003, 11)
    eng, _, _ = _fit_and_check(urm, "cosine", True, 1, {}, topk=3)
    eng.close()


@pytest.mark.parametrize("weighting", ["BM25", "TF-IDF"])
def test_fit_weighted_data(weighting):
    from ganmf_amd.ItemKNN import TF_IDF, okapi_BM_25
    base = _ratings(70, 50, 0.2, 1)
    fn = okapi_BM_25 if weighting == "BM25" else TF_IDF
    urm = sps.csr_matrix(fn(base.T).T, dtype=np.float32)      # the device's data: float32
    assert urm.data.min() > 0
    for setting in (KIND_SETTINGS[0], KIND_SETTINGS[1], KIND_SETTINGS[5]):
        eng, _, _ = _fit_and_check(urm, *setting, topk=7, weighted=True)
        eng.close()


def test_ties_go_to_the_smaller_item_id():
    m = _ratings(40, 12, 0.4, 2).toarray()
    for c in (4, 7, 9):
        m[:, c] = m[:, 2]      # four identical item columns: 2, 4, 7, 9
    eng = _engine(sps.csr_matrix(m))
    X = m.astype(np.float64)
    norm = np.sqrt((X * X).sum(axis=0))
    eng.itemknn_fit(H.PRODUCT, 2, shrink=0.0, den_a=norm, den_b=norm)
    W = sps.csc_matrix(eng.item_similarity())
    assert sorted(W[:, 2].indices) == [4, 7] and sorted(W[:, 4].indices) == [2, 7]
    assert sorted(W[:, 7].indices) == [2, 4] and sorted(W[:, 9].indices) == [2, 4]
    for i in set(range(12)) - {2, 4, 7, 9}:      # to every other item the four twins are exactly tied: all of them kept, or the smaller ids
        kept = set(W[:, i].indices) & {2, 4, 7, 9}
        assert kept in (set(), {2}, {2, 4})
    eng.close()


def test_two_fits_return_the_same_bytes():
    urm = _ratings(5000, 300, 0.02, 4)
    eng = _engine(urm)
    X32 = sps.csc_matrix(urm, dtype=np.float64)
    norm = np.sqrt(np.asarray(X32.power(2).sum(axis=0)).ravel())
    out = []
    for _ in range(2):
        eng.itemknn_fit(H.PRODUCT, 40, shrink=3.0, den_a=norm, den_b=norm)
        W = eng.item_similarity()
        out.append((W.indptr.tobytes(), W.indices.tobytes(), W.data.tobytes()))
    assert out[0] == out[1]
    other = _engine(urm)
    other.itemknn_fit(H.PRODUCT, 40, shrink=3.0, den_a=norm, den_b=norm)
    W = other.item_similarity()
    assert (W.indptr.tobytes(), W.indices.tobytes(), W.data.tobytes()) == out[0]
    eng.close()
    other.close()


# ---- scoring on its own --------------------------------------------------------------------------------------------------------
def _ragged_W(n_items, seed):
    """random non-negative W with ragged columns: an empty one, a full-length (or 3 000-long) one, the rest short"""
    rng = np.random.RandomState(seed)
    cols, rows, vals = [], [], []
    for i in range(n_items):
        length = 0 if i == n_items // 2 else (min(3000, n_items) if i == n_items // 3 else rng.randint(0, min(n_items, 40) + 1))
        j = rng.permutation(n_items)[:length] if length > 40 else np.unique(rng.randint(0, n_items, length))
        length = len(j)
        rows.extend(j.tolist())
        cols.extend([i] * length)
        vals.extend(rng.rand(length).tolist())
    return sps.csr_matrix((np.array(vals, dtype=np.float32), (rows, cols)), shape=(n_items, n_items))


@pytest.mark.parametrize("shape, density", [((70, 50), 0.2), ((90, 1), 0.3), ((90, 2), 0.3), ((90, 257), 0.3), ((60, 1100), 0.3),
                                            ((40000, 130), None), ((300, 33000), 0.003)], ids=lambda v: str(v))
def test_scores_of_an_uploaded_similarity(shape, density):
    urm = _ratings(shape[0], shape[1], density, 21, per_user=3 if density is None else None)
    W = _ragged_W(shape[1], 22)
    eng = _engine(urm)
    eng.set_item_similarity(W)
    back = eng.item_similarity()
    assert (back != W).nnz == 0
    X64, W64 = sps.csr_matrix(urm, dtype=np.float64), sps.csr_matrix(W, dtype=np.float64)
    Xp, Wp = X64.copy(), W64.copy()
    Xp.data[:] = 1.0
    Wp.data[:] = 1.0
    rng = np.random.RandomState(23)
    for ids in (np.array([shape[0] - 1]), rng.permutation(shape[0])[:7], np.arange(shape[0])):
        got = eng.scores(ids).astype(np.float64)
        want = np.asarray(X64[ids].dot(W64).todense())
        terms = np.asarray(Xp[ids].dot(Wp).todense())
        assert got.shape == want.shape
        bound = (terms + 2.0) * EPS * want
        assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) - bound).max())
        assert np.all(got[terms == 0] == 0.0)      # zeros where nothing is stored
    eng.close()


# ---- downstream routes at 70 x 50 ------------------------------------------------------------------------------------------------
def _host_twin(urm, W):
    """float64 scores from the device's own W behind the host evaluators and the host recommend()"""
    from ganmf_amd.base import BaseRecommender

    class Twin(BaseRecommender):
        def _compute_item_score(self, user_id_array, items_to_compute=None):
            s = H.scores(self.URM_train[np.asarray(user_id_array)], W)
            if items_to_compute is not None:
                keep = np.zeros(s.shape[1], dtype=bool)
                keep[np.asarray(items_to_compute)] = True
                s[:, ~keep] = -np.inf
            return s
    return Twin(urm)


@pytest.fixture(scope="module")
def fitted():
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender
    urm = _ratings(70, 50, 0.2, 1).tolil()
    urm[9, :] = 0      # a cold user
    urm = sps.csr_matrix(urm, dtype=np.float32)
    urm.eliminate_zeros()
    model = ItemKNNCFRecommender(urm)
    model.fit(topK=49, shrink=2, similarity="cosine", normalize=True)
    W = model.W_sparse
    twin = _host_twin(urm, W)
    rng = np.random.RandomState(31)
    t = (rng.rand(70, 50) < 0.15) * rng.randint(1, 6, size=(70, 50))
    t[9] = 0
    t[rng.rand(70) < 0.1] = 0
    test = sps.csr_matrix(t.astype(np.float32))
    yield model, twin, urm, test
    model.engine.close()


def _clear_ranks(twin, users, cutoff, remove_seen, items=None, ignore=()):
    """users whose cutoff-th and (cutoff+1)-th float64 scores are further apart than the fp32 scoring error, and their lists"""
    s = twin._compute_item_score(users, items_to_compute=items)
    if remove_seen:
        twin._remove_seen_on_scores_block(users, s)
    s[:, list(ignore)] = -np.inf
    order = np.argsort(-s, axis=1, kind="stable")
    ranked = np.take_along_axis(s, order, axis=1)
    tol = 64 * EPS * np.abs(ranked[:, :1] + 1e-30)
    gaps = np.abs(np.diff(ranked[:, :cutoff + 1], axis=1))
    finite = np.isfinite(ranked[:, :cutoff + 1])
    clear = np.all((gaps > tol) | ~(finite[:, :-1] & finite[:, 1:]), axis=1)
    lists = [order[r, :cutoff][np.isfinite(ranked[r, :cutoff])].tolist() for r in range(len(users))]
    return clear, lists


@pytest.mark.parametrize("remove_seen", [True, False])
def test_recommend_routes(fitted, remove_seen):
    model, twin, urm, _ = fitted
    users = np.arange(70)
    for kw, tw in ((dict(), dict()), (dict(items_to_compute=np.arange(0, 50, 2)), dict(items=np.arange(0, 50, 2)))):
        clear, want = _clear_ranks(twin, users, 5, remove_seen, **tw)
        got = model.recommend(users, cutoff=5, remove_seen_flag=remove_seen, **kw)
        assert clear.sum() > 50
        for u in np.flatnonzero(clear):
            assert got[u] == want[u], (u, got[u], want[u])
    model.set_items_to_ignore([0, 1, 2, 3])
    clear, want = _clear_ranks(twin, users, 5, remove_seen, ignore=(0, 1, 2, 3))
    got = model.recommend(users, cutoff=5, remove_seen_flag=remove_seen, remove_CustomItems_flag=True)
    for u in np.flatnonzero(clear):
        assert got[u] == want[u] and not set(got[u]) & {0, 1, 2, 3}
    model.reset_items_to_ignore()
    # a cold user scores zeros: ids, not -1 (ties to the smaller id)
    items = model.recommend_topk(np.array([9]), 5, remove_seen_flag=remove_seen)
    assert items[0].tolist() == [0, 1, 2, 3, 4]
    assert np.all(model._compute_item_score(np.array([9])) == 0.0)


def test_scores_of_the_class_equal_float64_from_its_own_W(fitted):
    model, twin, urm, _ = fitted
    users = np.arange(70)
    got, want = model._compute_item_score(users).astype(np.float64), twin._compute_item_score(users)
    assert np.all(np.abs(got - want) <= (49 + 2) * EPS * want)
    sub = model._compute_item_score(users, items_to_compute=[4, 6])
    assert np.all(np.isneginf(np.delete(sub, [4, 6], axis=1))) and np.array_equal(sub[:, [4, 6]], got[:, [4, 6]].astype(np.float32))


@pytest.mark.parametrize("full", [False, True])
def test_evaluators_on_the_device_equal_the_host_evaluators(fitted, full):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    model, twin, urm, test = fitted
    cut = [1, 5, 10]
    ev = EvaluatorHoldoutFast(test, cut, full_metrics=full)
    users = np.asarray(ev.usersToEvaluate)
    clear, _ = _clear_ranks(twin, users, 10, True)
    assert clear.all(), "pick another seed: a user's 10th and 11th scores are within the scoring error"
    assert ev.use_device_metrics
    dev, _ = ev.evaluateRecommender(model)
    host, _ = EvaluatorHoldoutFast(test, cut, full_metrics=full).evaluateRecommender(twin)
    for c in cut:
        assert set(dev[c]) == set(host[c])
        for name, v in host[c].items():
            if name == "RMSE" and not full:      # formed by the full row only
                assert np.isnan(dev[c][name]) and np.isnan(v)
                continue
            tol = 1e-5 if name == "RMSE" else 1e-12      # (RMSE: fp32 scores on the device, float64 on the host)
            assert abs(dev[c][name] - v) <= tol * max(1.0, abs(v)), (c, name, dev[c][name], v)
    assert host[5]["MAP"] > 0


def test_grouped_evaluation_on_the_device_equals_the_host(fitted):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    model, twin, urm, test = fitted
    groups = np.arange(70) % 3
    groups[::11] = -1
    dev = EvaluatorHoldoutFast(test, [5, 10]).evaluateRecommenderByGroup(model, groups)
    host = EvaluatorHoldoutFast(test, [5, 10]).evaluateRecommenderByGroup(twin, groups)
    assert set(dev) == set(host) == {0, 1, 2}
    for g in host:
        assert dev[g]["n_users"] == host[g]["n_users"]
        for c in (5, 10):
            for name, v in host[g][c].items():
                assert abs(dev[g][c][name] - v) <= 1e-12 * max(1.0, abs(v)), (g, c, name)


def test_save_load_scores_bit_for_bit(fitted, tmp_path):
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender
    model, _, urm, _ = fitted
    model.saveModel(str(tmp_path))
    other = ItemKNNCFRecommender(urm)
    other.loadModel(str(tmp_path))
    a, b = model.W_sparse, other.W_sparse
    assert a.indptr.tobytes() == b.indptr.tobytes() and a.indices.tobytes() == b.indices.tobytes() and a.data.tobytes() == b.data.tobytes()
    assert np.array_equal(model._compute_item_score(np.arange(70)), other._compute_item_score(np.arange(70)))
    other.engine.close()


def test_error_paths_leave_the_handle_usable():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = _ratings(70, 50, 0.2, 1)
    eng = _engine(urm)
    norm = np.ones(50)
    bad = [lambda: eng.itemknn_fit(6, 5), lambda: eng.itemknn_fit(-1, 5), lambda: eng.itemknn_fit(H.RAW, 0),
           lambda: eng.itemknn_fit(H.RAW, L.ITEMKNN_MAX_TOPK + 1), lambda: eng.itemknn_fit(H.RAW, 5, shrink=-1.0),
           lambda: eng.itemknn_fit(H.SHRINK_ONLY, 5, shrink=0.0), lambda: eng.itemknn_fit(H.PRODUCT, 5, den_a=norm),
           lambda: eng.itemknn_fit(H.TANIMOTO, 5), lambda: eng.scores(np.arange(3)),      # no W yet
           lambda: eng.item_similarity()]
    for call in bad:
        with pytest.raises(L.GanmfError):
            call()
    eng.itemknn_fit(H.PRODUCT, 5, den_a=norm, den_b=norm)
    W = eng.item_similarity()
    ref = eng.scores(np.arange(70))
    needs_tensors = [lambda: eng.train_epoch(np.arange(70)), lambda: eng.train_step(0, np.arange(1)), lambda: eng.get_tensor(L.T_USER_EMB),
                     lambda: eng.set_tensor(L.T_ITEM_EMB, np.zeros((50, 1))), lambda: eng.snapshot_best(), lambda: eng.restore_best(),
                     lambda: eng.als_half_sweep(0, 0.1), lambda: eng.pure_svd(np.zeros((50, 1)), 1), lambda: eng.discriminate(np.arange(2)),
                     lambda: eng.score_similarity(np.arange(4)), lambda: eng.bench_scores(4),
                     lambda: eng.recommend_candidates(np.arange(2), 3)]
    for call in needs_tensors:
        with pytest.raises(L.GanmfError, match="ITEMSIM"):
            call()
    with pytest.raises(L.GanmfError, match="transposed"):
        eng.scores(np.arange(3), transposed=True)
    with pytest.raises(L.GanmfError, match="transposed"):
        eng.recommend(np.arange(3), 5, transposed=True)
    with pytest.raises(L.GanmfError):
        eng.set_item_similarity(sps.csr_matrix(([np.nan], ([0], [1])), shape=(50, 50)))
    with pytest.raises(ValueError):
        eng.set_item_similarity(sps.identity(49, format="csr"))
    # a fit refused for its arguments keeps the matrix the handle holds
    with pytest.raises(L.GanmfError):
        eng.itemknn_fit(H.RAW, 0)
    assert (eng.item_similarity() != W).nnz == 0 and np.array_equal(eng.scores(np.arange(70)), ref)
    # a side that is not canonical, a missing side, a handle of another model
    half = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM)
    half.set_confidence(0, sps.csr_matrix(urm))
    with pytest.raises(L.GanmfError, match="side 1"):
        half.itemknn_fit(H.RAW, 5)
    t = sps.csr_matrix(urm).T.tocsr()
    t.sort_indices()
    at = t.indptr[np.flatnonzero(np.diff(t.indptr) >= 2)[0]]
    idx = t.indices.copy()
    idx[[at, at + 1]] = idx[[at + 1, at]]      # one row whose first two users descend
    half.set_confidence(1, sps.csr_matrix((t.data, idx, t.indptr), shape=t.shape))
    with pytest.raises(L.GanmfError, match="canonical"):
        half.itemknn_fit(H.RAW, 5)
    half.close()
    dp = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM, world_size=2, rank=0)      # a data-parallel handle
    dp.comm_init_local(7301)
    with pytest.raises(L.GanmfError, match="single-GPU"):
        dp.itemknn_fit(H.RAW, 5)
    dp.close()
    mf = Engine(70, 50, 2, 1, 1, model=L.MODEL_MF)
    with pytest.raises(L.GanmfError, match="ITEMSIM"):
        mf.itemknn_fit(H.RAW, 5)
    with pytest.raises(L.GanmfError, match="ITEMSIM"):
        mf.set_item_similarity(W)
    mf.close()
    eng.close()


# ---- known answers: the reference's logged ML-1M trials -------------------------------------------------------------------------
def _trial_doc():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "itemknn_trial_logs_ml1m.json")))


# the fixture's normalize: true trials and the five best-parameter rows
_TRIALS = [t for t in _trial_doc()["trials"] if t["params"]["normalize"] or t["role"] == "best"]


@pytest.fixture(scope="module")
def ml1m(golden_dir):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    doc = _trial_doc()
    train = sps.load_npz(os.path.join(golden_dir, doc["train"])).tocsr()
    valid = sps.load_npz(os.path.join(golden_dir, doc["validation"])).tocsr()
    return train, EvaluatorHoldoutFast(valid, [5])


def test_trial_selection():
    assert len(_TRIALS) >= 16 and sum(t["role"] == "best" for t in _TRIALS) == 5
    assert {t["kind"] for t in _TRIALS} == {"cosine", "asymmetric", "jaccard", "dice", "tversky"}


@pytest.mark.parametrize("n", range(len(_TRIALS)), ids=lambda n: "%s-%s-%d" % (_TRIALS[n]["kind"], _TRIALS[n]["role"], n))
def test_logged_trial_replayed_on_the_device(ml1m, n):
    """MAP@5 of one logged ML-1M trial through the class and EvaluatorHoldoutFast(validation, [5]).  The device has the latitude
    two implementations of the reference show among themselves (tie-breaking, rounding): |device - replayed| <= the largest
    |logged - replayed| among these trials in the fixture, + 1e-6 for the log's seven digits."""
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender
    train, ev = ml1m
    bound = max(abs(t["logged"] - t["replayed"]) for t in _TRIALS) + 1e-6
    t = _TRIALS[n]
    model = ItemKNNCFRecommender(train)
    model.fit(**t["params"])
    results, _ = ev.evaluateRecommender(model)
    model.engine.close()
    got = results[5]["MAP"]
    print("itemknn trial %-10s %-5s topK %4d shrink %4d: device %.7f replayed %.7f logged %.7f  |device - replayed| %.2e  "
          "|logged - replayed| %.2e  bound %.2e" % (t["kind"], t["role"], t["params"]["topK"], t["params"]["shrink"], got, t["replayed"],
                                                     t["logged"], abs(got - t["replayed"]), abs(t["logged"] - t["replayed"]), bound))
    assert abs(got - t["replayed"]) <= bound
