"""P3alpha / RP3beta on the device (ganmf_p3_fit on a GANMF_MODEL_ITEMSIM handle) against the float64 restatement of
tests/helpers_p3.py, fed the DEVICE'S OWN float32 inputs (the rounded transition terms), so only kernel rounding is under test.

Row pass (col_topk = 0, normalize = 0): R is checked for VALIDITY with the check of test_gpu_itemknn._check_sparse turned to rows, no
case left out: row i holds min(topK, number of non-zero w) entries, no duplicate, no self entry; every stored (j, v) has
|v - w64[i, j]| <= tau; the values sorted descending equal the helper's top values within tau.  tau = (len_i + 16) * 2^-24 * |v| with
len_i the stored count of column i: w_j is a chain of at most len_i FMAs with non-negative terms (one rounding each; the users outside
column i add exact zeros), then the scale multiply; the 16 is the slack of the weighted-data bound of the ItemKNN tests.
Normalisation: R(normalize = 1) against R(normalize = 0) divided by its float64 row sums, within (cnt_i + 2) * 2^-24 * |v|.
Column pass: moves values only, so it is checked EXACTLY (indptr, indices and data bytes) against helpers_p3.select_columns applied on
the host to the device's own col_topk = 0 output.
Scores: |device - float64 URM . W| <= (L + 2) * 2^-24 * score, L the number of terms of that score (non-negative operands)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_p3 as H
from tests.test_gpu_itemknn import _check_sparse, _clear_ranks, _edge_matrix, _host_twin, _ratings

pytestmark = pytest.mark.gpu

EPS = H.EPS32
F32 = np.float32


# ---- engines ------------------------------------------------------------------------------------------------------------------------
def _terms32(urm, alpha, beta=None):
    """the transition terms as the device receives them: formed in float64, rounded to float32 once"""
    rs, pui, cs = H.transition_terms(urm, alpha, beta)
    return rs.astype(F32), pui.astype(F32), None if cs is None else cs.astype(F32)


def _engine(urm, pui32):
    """a GANMF_MODEL_ITEMSIM engine holding `urm` as side 0 and the transition weights by item as side 1"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = H.canonical(sps.csr_matrix(urm, dtype=F32))
    eng = Engine(urm.shape[0], urm.shape[1], 1, 1, 1, model=L.MODEL_ITEMSIM)
    eng.set_confidence(0, urm)
    eng.set_confidence(1, pui32)
    eng.set_seen(urm)
    return eng


def _w64(rs32, pui32, cs32):
    return H.rows_sparse(rs32.astype(np.float64), pui32.astype(np.float64), None if cs32 is None else cs32.astype(np.float64))


def _same_bytes(a, b):
    a, b = sps.csr_matrix(a), sps.csr_matrix(b)
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and \
        a.data.dtype == b.data.dtype == F32 and a.data.tobytes() == b.data.tobytes()


def _rows_and_check(urm, topk, alpha, beta=None):
    """the row pass alone on a fresh engine, checked against the helper; returns (engine, R, the terms)"""
    rs, pui, cs = _terms32(urm, alpha, beta)
    eng = _engine(urm, pui)
    nnz = eng.p3_fit(topk, rs, col_scale=cs, normalize=False, col_topk=0)
    R = eng.item_similarity()
    assert R.nnz == nnz and R.dtype == F32 and R.has_sorted_indices
    w = _w64(rs, pui, cs)
    tau = (np.diff(pui.indptr) + 16.0) * EPS
    # _check_sparse works on columns: row i of R and of w are column i of their transposes
    wt = sps.csc_matrix(w.T)
    wt.sort_indices()
    worst = _check_sparse(sps.csr_matrix(R).T, wt, topk, tau)
    print("p3 rows alpha=%s beta=%s topK=%d: %d x %d, nnz %d, worst error / tau %.3f" % (alpha, beta, topk, urm.shape[0], urm.shape[1],
                                                                                        nnz, worst))
    return eng, R, (rs, pui, cs)


def _columns_check(eng, R, terms, topk, col_topk, normalize=False):
    """the fit with the column pass against select_columns of the device's own stage-1 output, exactly"""
    rs, pui, cs = terms
    stage1 = R
    if normalize:
        eng.p3_fit(topk, rs, col_scale=cs, normalize=True, col_topk=0)
        stage1 = eng.item_similarity()
    want = H.select_columns(stage1, col_topk)
    cut = int((np.diff(sps.csc_matrix(stage1).indptr) > col_topk).sum())
    nnz = eng.p3_fit(topk, rs, col_scale=cs, normalize=normalize, col_topk=col_topk)
    got = eng.item_similarity()
    assert got.nnz == nnz == want.nnz
    assert _same_bytes(got, want)
    return cut, stage1.nnz, nnz


# ---- the row pass against the helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, 0.6], ids=["p3alpha", "rp3beta"])
@pytest.mark.parametrize("alpha", [1.0, 0.7])
@pytest.mark.parametrize("topk", [1, 5, 49, 50, 1000])
def test_rows_every_topk_alpha_and_scale(topk, alpha, beta):
    eng, R, _ = _rows_and_check(_ratings(70, 50, 0.2, 1), topk, alpha, beta)
    assert 0 < np.diff(R.indptr).max() <= min(topk, 49)
    eng.close()


def _edge_with_a_stored_zero():
    urm = _edge_matrix()
    urm.data[urm.indptr[30]] = 0.0      # user 30's first rating: stored, zero
    assert urm.nnz == _edge_matrix().nnz and (urm.data == 0).sum() == 1
    return urm


@pytest.mark.parametrize("beta", [None, 0.6], ids=["p3alpha", "rp3beta"])
def test_rows_structural_edges(beta):
    urm = _edge_with_a_stored_zero()
    item = urm.indices[urm.indptr[30]]
    for topk in (1, 5, 50):
        eng, R, (rs, pui, _) = _rows_and_check(urm, topk, 0.7, beta)
        assert R[3, :].nnz == 0 and R[:, 3].nnz == 0      # the empty item: no row, in nobody's row
        assert R[13, :].nnz == min(topk, 2) and set(R[13, :].indices) <= {14, 15}
        assert R[8, :].nnz == min(topk, urm[11, :].nnz - 1)      # the one-entry column walks to its one user's other items
        # the stored zero counts in its item's degree and carries no weight of its own
        assert rs[item] == F32((1.0 / np.diff(sps.csc_matrix(urm).indptr)[item]) ** 0.7) and pui[item, 30] == 0
        eng.close()


@pytest.mark.parametrize("n_items", [1, 2, 257])
def test_rows_small_and_multi_block_catalogues(n_items):
    urm = _ratings(90, n_items, 0.3, n_items)
    for alpha, beta in ((1.0, None), (0.7, 0.6)):
        eng, R, terms = _rows_and_check(urm, 5, alpha, beta)
        if n_items == 1:
            assert R.nnz == 0
        cut, before, after = _columns_check(eng, R, terms, 5, 5, normalize=True)
        if n_items == 257:
            assert cut > 0 and after < before
        eng.close()


def test_rows_topk_1000_of_1100_items():
    eng, R, _ = _rows_and_check(_ratings(60, 1100, 0.3, 5), 1000, 0.7, 0.6)
    assert np.diff(R.indptr).max() == 1000
    eng.close()


def test_rows_more_users_than_one_lds_slab():
    urm = _ratings(40000, 130, None, 9, per_user=3)
    for alpha, beta in ((1.0, None), (0.7, 0.6)):
        eng, _, _ = _rows_and_check(urm, 20, alpha, beta)
        eng.close()


def test_row_above_the_lds_cap_in_both_passes():
    urm = _ratings(300, 33000, 0.003, 11)
    eng, R, terms = _rows_and_check(urm, 3, 0.7, 0.6)
    cut, before, after = _columns_check(eng, R, terms, 3, 3)
    print("p3 columns at 33000 items: %d columns cut, %d -> %d entries" % (cut, before, after))
    assert cut > 0 and after < before
    eng.close()


# ---- normalisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, topk", [((70, 50), 5), ((70, 50), 49), ((60, 1100), 1000)], ids=str)
def test_row_normalisation(shape, topk):
    urm = _ratings(shape[0], shape[1], 0.2 if shape[1] == 50 else 0.3, 1)
    rs, pui, cs = _terms32(urm, 0.7, 0.6)
    eng = _engine(urm, pui)
    eng.p3_fit(topk, rs, col_scale=cs, normalize=False, col_topk=0)
    R0 = eng.item_similarity()
    eng.p3_fit(topk, rs, col_scale=cs, normalize=True, col_topk=0)
    R1 = eng.item_similarity()
    assert np.array_equal(R0.indptr, R1.indptr) and np.array_equal(R0.indices, R1.indices)
    cnt = np.repeat(np.diff(R0.indptr), np.diff(R0.indptr)).astype(np.float64)
    want = H.normalize_rows(R0).data
    err = np.abs(R1.data.astype(np.float64) - want)
    assert np.all(err <= (cnt + 2) * EPS * np.abs(want)), float((err / ((cnt + 2) * EPS * np.abs(want))).max())
    sums = np.asarray(sps.csr_matrix(R1, dtype=np.float64).sum(axis=1)).ravel()
    kept = np.diff(R1.indptr) > 0
    assert kept.sum() > 0 and np.all(np.abs(sums[kept] - 1.0) <= (np.diff(R1.indptr)[kept] + 2) * EPS)
    assert np.all(sums[~kept] == 0)
    print("p3 normalise %s topK=%d: worst error / bound %.3f" % (shape, topk, float((err / ((cnt + 2) * EPS * np.abs(want))).max())))
    eng.close()


# ---- the column pass, exactly ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("topk", [5, 1])
def test_column_pass_moves_the_bytes_of_stage_one(topk, normalize):
    eng, R, terms = _rows_and_check(_ratings(70, 50, 0.2, 1), topk, 0.7)
    cut, before, after = _columns_check(eng, R, terms, topk, topk, normalize=normalize)
    print("p3 columns topK=%d normalize=%s: %d of 50 columns cut, %d -> %d entries" % (topk, normalize, cut, before, after))
    assert cut > 5 and after < before      # the pass has something to do
    # a column selection wider than any column keeps everything: the transposed stage one, as col_topk = 0 stores it
    assert _columns_check(eng, R, terms, topk, 50, normalize=normalize)[2] == before
    eng.close()


def test_column_pass_at_the_structural_edges():
    urm = _edge_with_a_stored_zero()
    for topk, col_topk in ((5, 5), (50, 3), (3, 1000)):
        eng, R, terms = _rows_and_check(urm, topk, 0.7, 0.6)
        _columns_check(eng, R, terms, topk, col_topk, normalize=True)
        W = eng.item_similarity()
        assert W[3, :].nnz == 0 and W[:, 3].nnz == 0
        eng.close()


# ---- ties and determinism ----------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_item_id_in_both_selections():
    m = _ratings(40, 12, 0.4, 2).toarray()
    for c in (4, 7, 9):
        m[:, c] = m[:, 2]      # four identical item columns: 2, 4, 7, 9
    urm = sps.csr_matrix(m)
    twins, prefixes = [2, 4, 7, 9], ([], [2], [2, 4], [2, 4, 7], [2, 4, 7, 9])
    others = sorted(set(range(12)) - set(twins))
    rs, pui, cs = _terms32(urm, 0.7, 0.6)
    eng = _engine(urm, pui)
    seen = set()
    for topk in (1, 2, 3, 5):      # rows: to every other item the four twins are exactly tied
        eng.p3_fit(topk, rs, col_scale=cs, normalize=False, col_topk=0)
        R = eng.item_similarity()
        for i in others:
            kept = sorted(set(R[i, :].indices) & set(twins))
            assert kept in prefixes, (topk, i, kept)
            seen.add(len(kept))
    assert seen - {0, 4}      # some row was cut inside the tie
    seen = set()
    for col_topk in (1, 2, 3, 5):      # columns: the four twin rows hold the same value in every other column (no row is cut: topk = 12)
        eng.p3_fit(12, rs, col_scale=cs, normalize=False, col_topk=col_topk)
        W = sps.csc_matrix(eng.item_similarity())
        for j in others:
            kept = sorted(set(W[:, j].indices) & set(twins))
            assert kept in prefixes, (col_topk, j, kept)
            seen.add(len(kept))
    assert seen - {0, 4}
    eng.close()


def test_two_fits_return_the_same_bytes():
    urm = _ratings(5000, 300, 0.02, 4)
    rs, pui, cs = _terms32(urm, 0.7, 0.6)
    eng = _engine(urm, pui)
    out = []
    for _ in range(2):
        eng.p3_fit(40, rs, col_scale=cs, normalize=True)
        out.append(eng.item_similarity())
    other = _engine(urm, pui)
    other.p3_fit(40, rs, col_scale=cs, normalize=True)
    out.append(other.item_similarity())
    assert out[0].nnz > 0 and _same_bytes(out[0], out[1]) and _same_bytes(out[0], out[2])
    eng.close()
    other.close()


# ---- downstream routes at 70 x 50, through the classes -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from ganmf_amd.P3 import P3alphaRecommender
    urm = _ratings(70, 50, 0.2, 1).tolil()
    urm[9, :] = 0      # a cold user
    urm = sps.csr_matrix(urm, dtype=F32)
    urm.eliminate_zeros()
    model = P3alphaRecommender(urm)
    model.fit(topK=20, alpha=0.7, normalize_similarity=True)
    W = model.W_sparse
    twin = _host_twin(urm, W)
    rng = np.random.RandomState(31)
    t = (rng.rand(70, 50) < 0.15) * rng.randint(1, 6, size=(70, 50))
    t[9] = 0
    t[rng.rand(70) < 0.1] = 0
    # users whose 10th and 11th float64 scores are inside the fp32 scoring error are not evaluated
    clear, _ = _clear_ranks(twin, np.arange(70), 10, True)
    t[~clear] = 0
    test = sps.csr_matrix(t.astype(F32))
    assert (np.diff(test.indptr) > 0).sum() > 50
    yield model, twin, urm, test
    model.engine.close()


def test_both_classes_fit_what_the_entry_fits_from_their_terms():
    """the classes' wiring on the device: W_sparse is, byte for byte, what ganmf_p3_fit returns for the class's own transition terms
    (col_scale only for RP3beta, the column selection at topK), and side 1 holds the ratings again afterwards"""
    from ganmf_amd.P3 import P3alphaRecommender, RP3betaRecommender, transition_terms
    urm = _ratings(70, 50, 0.2, 1)
    for cls, kw, beta in ((P3alphaRecommender, dict(topK=5, alpha=0.7, normalize_similarity=True), None),
                          (RP3betaRecommender, dict(topK=6, alpha=0.8, beta=0.4, normalize_similarity=False), 0.4)):
        model = cls(urm)
        model.fit(**kw)
        rs, pui, cs = transition_terms(urm, kw["alpha"], beta)
        assert (cs is None) == (beta is None)
        eng = _engine(urm, pui)
        eng.p3_fit(kw["topK"], rs, col_scale=cs, normalize=kw["normalize_similarity"], col_topk=kw["topK"])
        assert _same_bytes(model.W_sparse, eng.item_similarity())
        if beta is not None:      # the penalty changes the matrix
            eng.p3_fit(kw["topK"], rs, normalize=kw["normalize_similarity"], col_topk=kw["topK"])
            assert not _same_bytes(model.W_sparse, eng.item_similarity())
        W64 = sps.csr_matrix(model.W_sparse, dtype=np.float64)
        want = H.scores(urm, W64)
        got = model._compute_item_score(np.arange(70)).astype(np.float64)
        assert np.all(np.abs(got - want) <= (kw["topK"] + 2) * EPS * want)
        eng.close()
        model.engine.close()


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
    assert clear.sum() > 50
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
    Xp, Wp = sps.csr_matrix(urm, dtype=np.float64), sps.csr_matrix(model.W_sparse, dtype=np.float64)
    Xp.data[:] = 1.0
    Wp.data[:] = 1.0
    terms = np.asarray(Xp.dot(Wp).todense())
    assert want.max() > 0 and np.all(np.abs(got - want) <= (terms + 2) * EPS * want)
    assert np.all(got[terms == 0] == 0.0)
    sub = model._compute_item_score(users, items_to_compute=[4, 6])
    assert np.all(np.isneginf(np.delete(sub, [4, 6], axis=1))) and np.array_equal(sub[:, [4, 6]], got[:, [4, 6]].astype(F32))


@pytest.mark.parametrize("full", [False, True])
def test_evaluators_on_the_device_equal_the_host_evaluators(fitted, full):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    model, twin, urm, test = fitted
    cut = [1, 5, 10]
    ev = EvaluatorHoldoutFast(test, cut, full_metrics=full)
    assert len(ev.usersToEvaluate) > 50 and ev.use_device_metrics
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
    from ganmf_amd.P3 import P3alphaRecommender
    model, _, urm, _ = fitted
    model.saveModel(str(tmp_path))
    other = P3alphaRecommender(urm)
    other.loadModel(str(tmp_path))
    assert _same_bytes(model.W_sparse, other.W_sparse)
    assert np.array_equal(model._compute_item_score(np.arange(70)), other._compute_item_score(np.arange(70)))
    other.engine.close()


# ---- error paths ---------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_held_matrix_and_its_scores():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = _ratings(70, 50, 0.2, 1)
    rs, pui, cs = _terms32(urm, 0.7, 0.6)
    eng = _engine(urm, pui)
    for call in (lambda: eng.scores(np.arange(3)), lambda: eng.item_similarity()):      # no W yet
        with pytest.raises(L.GanmfError):
            call()
    eng.p3_fit(5, rs, col_scale=cs, normalize=True)
    W = eng.item_similarity()
    ref = eng.scores(np.arange(70))

    def spoiled(v, at, value):
        out = v.copy()
        out[at] = value
        return out
    bad = [lambda: eng.p3_fit(0, rs), lambda: eng.p3_fit(-3, rs), lambda: eng.p3_fit(L.ITEMKNN_MAX_TOPK + 1, rs),
           lambda: eng.p3_fit(5, rs, col_topk=-1), lambda: eng.p3_fit(5, rs, col_topk=L.ITEMKNN_MAX_TOPK + 1),
           lambda: eng.p3_fit(5, spoiled(rs, 7, -0.5)), lambda: eng.p3_fit(5, spoiled(rs, 49, np.nan)),
           lambda: eng.p3_fit(5, spoiled(rs, 0, np.inf)), lambda: eng.p3_fit(5, rs, col_scale=spoiled(cs, 3, -1.0)),
           lambda: eng.p3_fit(5, rs, col_scale=spoiled(cs, 3, np.nan)), lambda: eng.p3_fit(5, rs, col_scale=spoiled(cs, 48, np.inf))]
    for call in bad:
        with pytest.raises(L.GanmfError, match="ganmf_p3_fit"):
            call()
        assert _same_bytes(eng.item_similarity(), W) and np.array_equal(eng.scores(np.arange(70)), ref)
    needs_tensors = [lambda: eng.train_epoch(np.arange(70)), lambda: eng.train_step(0, np.arange(1)), lambda: eng.get_tensor(L.T_USER_EMB),
                     lambda: eng.set_tensor(L.T_ITEM_EMB, np.zeros((50, 1))), lambda: eng.snapshot_best(), lambda: eng.restore_best(),
                     lambda: eng.als_half_sweep(0, 0.1), lambda: eng.pure_svd(np.zeros((50, 1)), 1), lambda: eng.discriminate(np.arange(2)),
                     lambda: eng.score_similarity(np.arange(4)), lambda: eng.bench_scores(4),
                     lambda: eng.recommend_candidates(np.arange(2), 3)]
    for call in needs_tensors:
        with pytest.raises(L.GanmfError, match="ITEMSIM"):
            call()
    assert _same_bytes(eng.item_similarity(), W) and np.array_equal(eng.scores(np.arange(70)), ref)
    # the matrix is an ordinary held W: it can be read, uploaded again and scored
    eng.set_item_similarity(W)
    assert _same_bytes(eng.item_similarity(), W) and np.array_equal(eng.scores(np.arange(70)), ref)
    # a missing side, a side that is not canonical, a data-parallel handle, a handle of another model
    half = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM)
    half.set_confidence(0, sps.csr_matrix(urm))
    with pytest.raises(L.GanmfError, match="side 1"):
        half.p3_fit(5, rs)
    idx = pui.indices.copy()
    at = pui.indptr[np.flatnonzero(np.diff(pui.indptr) >= 2)[0]]
    idx[[at, at + 1]] = idx[[at + 1, at]]      # one row whose first two users descend
    half.set_confidence(1, sps.csr_matrix((pui.data, idx, pui.indptr), shape=pui.shape))
    with pytest.raises(L.GanmfError, match="canonical"):
        half.p3_fit(5, rs)
    half.close()
    only1 = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM)
    only1.set_confidence(1, pui)
    with pytest.raises(L.GanmfError, match="side 0"):
        only1.p3_fit(5, rs)
    only1.close()
    dp = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM, world_size=2, rank=0)      # a data-parallel handle
    dp.comm_init_local(7302)
    with pytest.raises(L.GanmfError, match="single-GPU"):
        dp.p3_fit(5, rs)
    dp.close()
    mf = Engine(70, 50, 2, 1, 1, model=L.MODEL_MF)
    with pytest.raises(L.GanmfError, match="ITEMSIM"):
        mf.p3_fit(5, rs)
    mf.close()
    eng.close()


# ---- known answers: the reference's logged ML-1M trials -------------------------------------------------------------------------
def _trial_doc():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p3_trial_logs_ml1m.json")))


_TRIALS = _trial_doc()["trials"]


@pytest.fixture(scope="module")
def ml1m(golden_dir):
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    doc = _trial_doc()
    train = sps.load_npz(os.path.join(golden_dir, doc["train"])).tocsr()
    valid = sps.load_npz(os.path.join(golden_dir, doc["validation"])).tocsr()
    return train, EvaluatorHoldoutFast(valid, [5])


@pytest.mark.parametrize("n", range(len(_TRIALS)), ids=lambda n: "%s-%d" % (_TRIALS[n]["role"], n))
def test_logged_trial_replayed_on_the_device(ml1m, n):
    """MAP@5 of one logged ML-1M trial through P3alphaRecommender and EvaluatorHoldoutFast(validation, [5]):
    |device - restated64| <= 4 * latitude + 1e-6.  latitude is measured on the CPU between the reference and two roundings of its own
    arithmetic (the float64 and the float32 restatement) and its log; the device is a third rounding (FMA chains, host-formed
    powers) under the tie rule of restated64; the factor 4 covers the small sample of four rows, 1e-6 the log's seven digits.  The
    bound stays below 1 / (2 * 6040): one user's list going wrong moves MAP@5 by more."""
    from ganmf_amd.P3 import P3alphaRecommender
    train, ev = ml1m
    doc = _trial_doc()
    bound = 4 * doc["latitude"] + 1e-6
    t = _TRIALS[n]
    model = P3alphaRecommender(train.copy())
    model.fit(**t["params"])
    results, _ = ev.evaluateRecommender(model)
    model.engine.close()
    got = results[5]["MAP"]
    print("p3alpha trial %-5s topK %4d alpha %.4f normalize %-5s: device %.7f restated64 %.7f replayed %.7f logged %.7f  "
          "|device - restated64| %.2e  bound %.2e" % (t["role"], t["params"]["topK"], t["params"]["alpha"],
                                                      t["params"]["normalize_similarity"], got, t["restated64"], t["replayed"],
                                                      t["logged"], abs(got - t["restated64"]), bound))
    assert abs(got - t["restated64"]) <= bound
