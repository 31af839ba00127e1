"""User-KNN on the device (ganmf_userknn_fit / ganmf_set_user_similarity / userknn_score_kernel behind the scores of a
GANMF_MODEL_ITEMSIM handle) against the float64 restatement of tests/helpers_userknn.py.

Fit: W is checked for VALIDITY per column (the target user), by the four conditions of tests/test_gpu_itemknn.py::_check_sparse
restated here over a block of columns (_check_columns): a column holds min(topK, number of non-zero similarities) entries, no
duplicate, no self entry; every stored (j, v) has |v - sim64[j, i]| <= tau; the values sorted descending equal the helper's top values
within tau.  The bounds are that file's: on integer-valued matrices every dot product is an integer below 2^24, exact in fp32, and the
value is at most eight fp32 roundings away, tau = 16 * 2^-24 * |v|; on BM25 / TF-IDF data the FMA chain over the len_i entries of user
i's profile adds len_i roundings, tau = (len_i + 16) * 2^-24 * |v|.
Scores: out[u, i] = sum_v W[u, v] R[v, i] is one fp32 FMA chain of m terms: every partial sum s_k = (s_{k-1} + t_k)(1 + d_k) with
|d_k| <= 2^-24 (one rounding per FMA), so |dev - exact| <= m * 2^-24 * sum|w r| to first order; the operands are the device's own
float32 values, and two further units cover the second-order terms and the float64 reference: (m + 2) * 2^-24 * sum|w r|.  Derived,
not measured.  Exactly 0 where m = 0."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_itemknn as HI
from tests import helpers_userknn as H

pytestmark = pytest.mark.gpu

EPS = H.EPS32


# ---- matrices and engines -------------------------------------------------------------------------------------------------------
def _ratings(n_users, n_items, density, seed, per_user=None):
    """integer ratings 1..5 (tests/test_gpu_itemknn.py::_ratings, restated)"""
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
    """70 x 50 at density 0.2 with an empty user (3), an empty item (5), a one-entry user (8, item 11), and a user (13) with fewer
    co-raters than topK = 5: the only other raters of its two items 20 and 21 are users 14 and 15"""
    m = _ratings(70, 50, 0.2, 7).tolil()
    m[3, :] = 0
    m[:, 5] = 0
    m[8, :] = 0
    m[8, 11] = 4
    m[:, 20] = 0
    m[:, 21] = 0
    m[13, :] = 0
    m[13, 20], m[14, 20] = 2, 3
    m[13, 21], m[15, 21] = 5, 1
    m = sps.csr_matrix(m, dtype=np.float32)
    m.eliminate_zeros()
    return m


def _engine(urm, binarise=False):
    """a GANMF_MODEL_ITEMSIM engine holding `urm` on side 0 (as ones when the similarity binarises); side 1 is not uploaded: the
    user fit and the user scores do not read it"""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = sps.csr_matrix(urm, dtype=np.float32)
    urm.sort_indices()
    eng = Engine(urm.shape[0], urm.shape[1], 1, 1, 1, model=L.MODEL_ITEMSIM)
    seen = urm.copy()
    if binarise:
        seen.data[:] = 1.0
    eng.set_confidence(0, seen)
    eng.set_seen(urm)
    return eng


def _similarity_block(Xt, c0, c1, kind, shrink, p0, p1, den_a, den_b):
    """The float64 similarities of the target users [c0, c1) with every user at the non-zero dot products (CSC [users, c1 - c0], no
    self entry): tests/test_gpu_itemknn.py::_sparse_similarity over a block of columns.  Xt: items x users, CSC float64."""
    w = sps.csc_matrix(Xt.T.dot(Xt[:, c0:c1]))
    w.sort_indices()
    j = w.indices
    i = np.repeat(np.arange(c0, c1), np.diff(w.indptr))
    v = np.where(i == j, 0.0, w.data)
    s = float(shrink) + 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == HI.PRODUCT:
            v = v / (den_a[i] * den_b[j] + s)
        elif kind == HI.TANIMOTO:
            v = v / (den_a[i] + den_a[j] - v + s)
        elif kind == HI.DICE:
            v = v / (den_a[i] + den_a[j] + s)
        elif kind == HI.TVERSKY:
            v = v / (v + (den_a[i] - v) * p0 + (den_a[j] - v) * p1 + s)
        elif kind == HI.SHRINK_ONLY:
            v = v / float(shrink)
    out = sps.csc_matrix((v, j, w.indptr), shape=w.shape)
    out.eliminate_zeros()
    return out


def _check_columns(W, sim, c0, topk, tau_scale):
    """The four conditions of the module's docstring for the columns [c0, c0 + sim.shape[1]) of the device's W (CSC, sorted) against
    the float64 block `sim`; tau_scale[i] * |v| is column i's bound.  Returns the largest error / bound seen."""
    k = min(topk, W.shape[0])
    worst = 0.0
    for c in range(sim.shape[1]):
        i = c0 + c
        idx = W.indices[W.indptr[i]:W.indptr[i + 1]]
        val = W.data[W.indptr[i]:W.indptr[i + 1]].astype(np.float64)
        ref_j = sim.indices[sim.indptr[c]:sim.indptr[c + 1]]
        ref_v = sim.data[sim.indptr[c]:sim.indptr[c + 1]]
        if len(ref_v) > 4 * k:      # (the same k entries, sorting only those at or above the k-th largest value)
            cand = np.flatnonzero(ref_v >= np.partition(ref_v, -k)[-k])
            keep = cand[np.lexsort((ref_j[cand], -ref_v[cand]))[:k]]
        else:
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


def _plan(urm, similarity, normalize, shrink, asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0):
    """helpers_userknn.host_plan without its dense copy: (kind, p0, p1, den_a, den_b), the den per user in float64"""
    kind = {"jaccard": HI.TANIMOTO, "tanimoto": HI.TANIMOTO, "dice": HI.DICE, "tversky": HI.TVERSKY}.get(similarity)
    m = sps.csr_matrix(urm, dtype=np.float64)
    if kind is not None:
        return kind, float(tversky_alpha), float(tversky_beta), np.diff(m.indptr).astype(np.float64), None
    if normalize:
        norm = np.sqrt(np.asarray(m.power(2).sum(axis=1)).ravel())
        if similarity == "asymmetric":
            return HI.PRODUCT, 1.0, 1.0, np.power(norm, 2 * asymmetric_alpha), np.power(norm, 2 * (1 - asymmetric_alpha))
        return HI.PRODUCT, 1.0, 1.0, norm, norm
    return (HI.SHRINK_ONLY if shrink != 0 else HI.RAW), 1.0, 1.0, None, None


def _fit_and_check(urm, similarity, normalize, shrink, extra, topk, weighted=False, block=1024):
    kind, p0, p1, den_a, den_b = _plan(urm, similarity, normalize, shrink, **extra)
    n = urm.shape[0]
    if n <= 2000:      # the sparse plan is the helper's
        ref = H.host_plan(urm, similarity, normalize, shrink, **extra)
        assert ref[0] == kind and (ref[2], ref[3]) == (p0, p1)
        for a, b in ((den_a, ref[4]), (den_b, ref[5])):
            assert (a is None) == (b is None) and (a is None or np.allclose(a, b, rtol=1e-14, atol=0))
    binarise = kind in (HI.TANIMOTO, HI.DICE, HI.TVERSKY)
    eng = _engine(urm, binarise)
    seen = sps.csr_matrix(urm, dtype=np.float32, copy=True)
    if binarise:
        seen.data[:] = 1.0
    a32 = None if den_a is None else den_a.astype(np.float32)
    b32 = None if den_b is None else den_b.astype(np.float32)
    nnz = eng.userknn_fit(kind, topk, shrink=shrink, p0=p0, p1=p1, den_a=a32, den_b=b32)
    W = eng.user_similarity()
    assert W.nnz == nnz and W.dtype == np.float32 and W.shape == (n, n)
    by_row = W.copy()
    by_row.sort_indices()
    assert by_row.indices.tobytes() == W.indices.tobytes()      # every row ascends as it comes from the device
    # the helper sees what the device sees: float32 data, float32 denominators, float32 coefficients
    lens = np.diff(seen.indptr)
    tau = (lens + 16.0) * EPS if weighted else np.full(n, 16.0 * EPS)
    Xt = sps.csc_matrix(seen.T, dtype=np.float64)
    Wc = sps.csc_matrix(W)
    Wc.sort_indices()
    worst = 0.0
    for c0 in range(0, n, block):
        sim = _similarity_block(Xt, c0, min(n, c0 + block), kind, np.float32(shrink), np.float32(p0), np.float32(p1),
                                None if a32 is None else a32.astype(np.float64), None if b32 is None else b32.astype(np.float64))
        worst = max(worst, _check_columns(Wc, sim, c0, topk, tau))
    print("userknn %s normalize=%s shrink=%s %s topK=%d: %d x %d, nnz %d, longest row %d, worst error / tau %.3f" % (
        similarity, normalize, shrink, extra, topk, urm.shape[0], urm.shape[1], nnz, int(np.diff(W.indptr).max()), worst))
    return eng, W


# ---- W against the helper ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topk", [1, 5, 69, 70, 1000])
@pytest.mark.parametrize("setting", KIND_SETTINGS, ids=lambda s: "%s-%s-%s" % s[:3])
def test_fit_every_kind_and_topk(setting, topk):
    eng, W = _fit_and_check(_ratings(70, 50, 0.2, 1), *setting, topk=topk)
    if topk == 5 and setting[0] == "cosine" and setting[1]:      # selected by column, read by row: a row is not bounded by topK
        assert np.diff(sps.csc_matrix(W).indptr).max() == 5 and np.diff(W.indptr).max() > 5
    eng.close()


@pytest.mark.parametrize("weighting", ["BM25", "TF-IDF"])
def test_fit_weighted_data(weighting):
    from ganmf_amd.knn_model import TF_IDF, okapi_BM_25
    base = _ratings(70, 50, 0.2, 1)
    fn = okapi_BM_25 if weighting == "BM25" else TF_IDF
    urm = sps.csr_matrix(fn(base.T).T, dtype=np.float32)      # the device's data: float32
    assert urm.data.min() > 0
    for setting in (KIND_SETTINGS[0], KIND_SETTINGS[1], KIND_SETTINGS[5]):
        eng, _ = _fit_and_check(urm, *setting, topk=7, weighted=True)
        eng.close()


@pytest.mark.parametrize("setting", KIND_SETTINGS, ids=lambda s: "%s-%s-%s" % s[:3])
def test_fit_structural_edges(setting):
    urm = _edge_matrix()
    raters_11 = set(np.flatnonzero(urm[:, 11].toarray().ravel())) - {8}
    assert len(raters_11) > 5 and urm[:, 5].nnz == 0 and urm[3].nnz == 0 and urm[8].nnz == 1
    for topk in (1, 5, 70):
        eng, W = _fit_and_check(urm, *setting, topk=topk)
        Wc = sps.csc_matrix(W)
        assert Wc[:, 3].nnz == 0 and W[3, :].nnz == 0      # the empty user: no neighbours, nobody's neighbour
        assert Wc[:, 13].nnz == min(topk, 2) and set(Wc[:, 13].indices) <= {14, 15}      # fewer co-raters than topK
        assert Wc[:, 8].nnz == min(topk, len(raters_11)) and set(Wc[:, 8].indices) <= raters_11      # the one-entry user
        assert set(W[13, :].indices) <= {14, 15} and set(W[8, :].indices) <= raters_11      # ... and the rows they can be in
        eng.close()


def test_raw_dot_products_are_exact_integers():
    urm = _ratings(70, 50, 0.2, 1)
    eng = _engine(urm)
    eng.userknn_fit(HI.RAW, 70)
    W = np.asarray(eng.user_similarity().todense(), dtype=np.float64)
    X = HI.dense64(urm)
    w = X.dot(X.T)
    np.fill_diagonal(w, 0.0)
    assert w.max() < 2 ** 24
    np.testing.assert_array_equal(W, w)      # all 69 neighbours kept: the whole (symmetric) matrix, exactly
    eng.close()


def test_fit_more_items_than_one_lds_slab():
    """the slab walk of the row builder with the sides exchanged: 9 000 items are more than one slab of 8 192"""
    urm = sps.csr_matrix(_ratings(9000, 130, None, 9, per_user=3).T)      # 130 users x 9 000 items, 3 entries per item
    assert urm.shape == (130, 9000)
    for setting in (KIND_SETTINGS[0], KIND_SETTINGS[4], KIND_SETTINGS[6]):
        eng, _ = _fit_and_check(urm, *setting, topk=20)
        eng.close()


def test_fit_row_above_the_lds_cap():
    """28 673 users are one past KNN_ROW_LDS: the similarity row lives in global memory.  No smaller shape crosses the limit; the
    float64 side forms 28 673 columns of about 4 500 non-zero similarities each, in blocks, which takes most of this test's time
    (several seconds)."""
    urm = _ratings(28673, 24, None, 11, per_user=2)
    eng, W = _fit_and_check(urm, "cosine", True, 1, {}, topk=3)
    assert np.diff(W.indptr).max() > 3
    eng.close()


def test_ties_go_to_the_smaller_user_id():
    m = _ratings(12, 40, 0.4, 2).toarray()
    for r in (4, 7, 9):
        m[r] = m[2]      # four identical users: 2, 4, 7, 9
    eng = _engine(sps.csr_matrix(m))
    X = m.astype(np.float64)
    norm = np.sqrt((X * X).sum(axis=1))
    eng.userknn_fit(HI.PRODUCT, 2, shrink=0.0, den_a=norm, den_b=norm)
    W = sps.csc_matrix(eng.user_similarity())
    assert sorted(W[:, 2].indices) == [4, 7] and sorted(W[:, 4].indices) == [2, 7]
    assert sorted(W[:, 7].indices) == [2, 4] and sorted(W[:, 9].indices) == [2, 4]
    eng.close()


def test_two_fits_return_the_same_bytes():
    urm = _ratings(300, 5000, 0.02, 4)
    norm = np.sqrt(np.asarray(sps.csr_matrix(urm, dtype=np.float64).power(2).sum(axis=1)).ravel())
    out = []
    for _ in range(2):
        eng = _engine(urm)
        for _ in range(2):
            eng.userknn_fit(HI.PRODUCT, 40, shrink=3.0, den_a=norm, den_b=norm)
            W = eng.user_similarity()
            out.append((W.indptr.tobytes(), W.indices.tobytes(), W.data.tobytes()))
        eng.close()
    assert out[0] == out[1] == out[2] == out[3]


# ---- the exact product ----------------------------------------------------------------------------------------------------------
def test_exact_product_scores_and_lists():
    """cosine, normalize=False, shrink=0: W holds the integer dot products (at most 50 * 25 = 1 250) and every score is an integer of
    at most 70 * 1 250 * 5 < 2^24, so every partial sum of the FMA chain is exact: the scores EQUAL float64, and so do the lists"""
    from ganmf_amd.UserKNN import UserKNNCFRecommender
    urm = _ratings(70, 50, 0.2, 1)
    model = UserKNNCFRecommender(urm)
    model.fit(topK=70, shrink=0, similarity="cosine", normalize=False)
    W = model.W_sparse
    want_W = H.fit(urm, topK=70, shrink=0, similarity="cosine", normalize=False)
    np.testing.assert_array_equal(W.toarray().astype(np.float64), want_W.toarray())
    users = np.arange(70)
    want = H.scores(urm, want_W)
    assert want.max() < 2 ** 24 and np.all(want == np.round(want))
    got = model._compute_item_score(users)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.astype(np.float64), want)
    for remove_seen in (False, True):
        s = want.copy()
        if remove_seen:
            s[urm.toarray() != 0] = -np.inf
        lists = H.ranked_lists(s, 10)
        assert model.recommend(users, cutoff=10, remove_seen_flag=remove_seen) == lists      # every user, ties to the smaller id
    model.engine.close()


# ---- the general product: an uploaded W -------------------------------------------------------------------------------------------
def _ragged_user_W(n_users, seed):
    """random W with values in (0, 1) and rows of length 0, 1, min(300, n_users - 1) and n_users - 1 among short random ones"""
    rng = np.random.RandomState(seed)
    fixed = {0: 0, 1: 1, 2: min(300, n_users - 1), 3: n_users - 1}
    rows, cols, vals = [], [], []
    for u in range(n_users):
        length = fixed.get(u, rng.randint(0, min(n_users, 40)))
        others = np.delete(np.arange(n_users), u)
        v = np.sort(rng.permutation(others)[:length])
        rows.extend([u] * len(v))
        cols.extend(v.tolist())
        vals.extend((rng.rand(len(v)) * 0.998 + 0.001).tolist())
    W = sps.csr_matrix((np.array(vals, dtype=np.float32), (rows, cols)), shape=(n_users, n_users))
    assert sorted({0, 1, fixed[2], n_users - 1}) == sorted(set(np.diff(W.indptr)[:4]))
    return W


def _wide_matrix():
    """300 x 33 000 (above KNN_SCORE_LDS: the accumulator is the output row) with a user who rated 20 000 items: thousands of entries
    inside every wave's range"""
    m = _ratings(300, 33000, 0.003, 11).tolil()
    rng = np.random.RandomState(12)
    for i in rng.permutation(33000)[:20000]:
        m[4, i] = rng.randint(1, 6)
    return sps.csr_matrix(m, dtype=np.float32)


@pytest.mark.parametrize("case", ["70x50", "60x1100", "300x33000", "40x1"])
def test_scores_of_an_uploaded_similarity(case):
    urm = {"70x50": lambda: _ratings(70, 50, 0.2, 21), "60x1100": lambda: _ratings(60, 1100, 0.3, 21), "300x33000": _wide_matrix,
           "40x1": lambda: _ratings(40, 1, 0.5, 21)}[case]()
    n_users = urm.shape[0]
    W = _ragged_user_W(n_users, 22)
    eng = _engine(urm)
    eng.set_user_similarity(W)
    back = eng.user_similarity()
    assert (back != W).nnz == 0 and back.indices.tobytes() == W.indices.tobytes() and back.data.tobytes() == W.data.tobytes()
    X64, W64 = sps.csr_matrix(urm, dtype=np.float64), sps.csr_matrix(W, dtype=np.float64)
    rng = np.random.RandomState(23)
    for ids in (np.array([n_users - 1]), np.concatenate([np.arange(4), rng.permutation(n_users)[:5]]), np.arange(n_users)):
        got = eng.scores(ids).astype(np.float64)
        want = H.scores(X64, W64, ids)
        m = H.terms(X64, W64, ids)
        mass = H.scores(abs(X64), abs(W64), ids)
        assert got.shape == want.shape == (len(ids), urm.shape[1])
        bound = (m + 2.0) * EPS * mass
        assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) - bound).max())
        assert np.all(got[m == 0] == 0.0) and not np.any(np.signbit(got[m == 0]))      # exactly 0.f where nothing is summed
        print("userknn scores %s, %d rows: most terms %d, worst error / bound %.3f" % (
            case, len(ids), int(m.max()), float((np.abs(got - want)[m > 0] / bound[m > 0]).max()) if (m > 0).any() else 0.0))
    eng.close()


def test_scores_do_not_depend_on_the_batch():
    urm = _ratings(70, 50, 0.2, 21)
    eng = _engine(urm)
    eng.set_user_similarity(_ragged_user_W(70, 22))
    every = eng.scores(np.arange(70))
    again = eng.scores(np.arange(70))
    assert every.tobytes() == again.tobytes()
    mixed = eng.scores(np.array([5, 5, 0, 69, 5]))
    for r, u in enumerate([5, 5, 0, 69, 5]):
        assert mixed[r].tobytes() == every[u].tobytes()
    for u in (0, 2, 3, 69):
        assert eng.scores(np.array([u]))[0].tobytes() == every[u].tobytes()
    eng.close()
    wide = _wide_matrix()      # the accumulator in the output row itself
    eng = _engine(wide)
    eng.set_user_similarity(_ragged_user_W(300, 22))
    every = eng.scores(np.arange(300))
    mixed = eng.scores(np.array([5, 5, 0, 299, 3]))
    for r, u in enumerate([5, 5, 0, 299, 3]):
        assert mixed[r].tobytes() == every[u].tobytes()
    assert eng.scores(np.array([3]))[0].tobytes() == every[3].tobytes()
    eng.close()


# ---- downstream routes at 70 x 50 ------------------------------------------------------------------------------------------------
def _host_twin(urm, W):
    """float64 scores from the device's own W behind the host evaluators and the host recommend()"""
    from ganmf_amd.base import BaseRecommender

    class Twin(BaseRecommender):
        def _compute_item_score(self, user_id_array, items_to_compute=None):
            s = H.scores(self.URM_train, W, user_id_array)
            if items_to_compute is not None:
                keep = np.zeros(s.shape[1], dtype=bool)
                keep[np.asarray(items_to_compute)] = True
                s[:, ~keep] = -np.inf
            return s
    return Twin(urm)


@pytest.fixture(scope="module")
def fitted():
    from ganmf_amd.UserKNN import UserKNNCFRecommender
    urm = _ratings(70, 50, 0.2, 5).tolil()      # (a seed at which no evaluated user's 10th and 11th float64 scores nearly tie)
    urm[9, :] = 0      # a cold user
    urm = sps.csr_matrix(urm, dtype=np.float32)
    urm.eliminate_zeros()
    model = UserKNNCFRecommender(urm)
    model.fit(topK=20, shrink=2, similarity="cosine", normalize=True)
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
    """users whose cutoff-th and (cutoff+1)-th float64 scores are further apart than the fp32 scoring error, and their lists
    (tests/test_gpu_itemknn.py::_clear_ranks)"""
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
    # a cold user has no neighbour and scores zeros: ids, not -1 (ties to the smaller id)
    items = model.recommend_topk(np.array([9]), 5, remove_seen_flag=remove_seen)
    assert items[0].tolist() == [0, 1, 2, 3, 4]
    assert np.all(model._compute_item_score(np.array([9])) == 0.0)


def test_scores_of_the_class_equal_float64_from_its_own_W(fitted):
    model, twin, urm, _ = fitted
    users = np.arange(70)
    W = model.W_sparse
    assert W.shape == (70, 70) and W.dtype == np.float32 and np.diff(sps.csc_matrix(W).indptr).max() == 20
    got, want = model._compute_item_score(users).astype(np.float64), twin._compute_item_score(users)
    assert np.all(np.abs(got - want) <= (H.terms(urm, W) + 2) * EPS * want)      # (non-negative operands: sum|w r| is the score)
    sub = model._compute_item_score(users, items_to_compute=[4, 6])
    assert np.all(np.isneginf(np.delete(sub, [4, 6], axis=1))) and np.array_equal(sub[:, [4, 6]], got[:, [4, 6]].astype(np.float32))
    np.testing.assert_array_equal(model.engine.scores(users), got.astype(np.float32))


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
    from ganmf_amd.UserKNN import UserKNNCFRecommender
    model, _, urm, _ = fitted
    model.saveModel(str(tmp_path))
    other = UserKNNCFRecommender(urm)
    other.loadModel(str(tmp_path))
    a, b = model.W_sparse, other.W_sparse
    assert a.indptr.tobytes() == b.indptr.tobytes() and a.indices.tobytes() == b.indices.tobytes() and a.data.tobytes() == b.data.tobytes()
    assert np.array_equal(model._compute_item_score(np.arange(70)), other._compute_item_score(np.arange(70)))
    other.engine.close()


def test_binarising_fit_scores_the_ratings():
    """jaccard puts ones into side 0 for the fit; the scores are formed from URM_train's own values"""
    from ganmf_amd.UserKNN import UserKNNCFRecommender
    urm = _ratings(70, 50, 0.2, 1)
    model = UserKNNCFRecommender(urm)
    model.fit(topK=10, shrink=1, similarity="jaccard")
    W = model.W_sparse
    got, want = model._compute_item_score(np.arange(70)).astype(np.float64), H.scores(urm, W)
    assert want.max() > 5 and np.all(np.abs(got - want) <= (H.terms(urm, W) + 2) * EPS * want)
    model.engine.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_handle_usable():
    """every call below is refused by a check in front of any launch"""
    import ctypes as C
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = _ratings(70, 50, 0.2, 1)
    eng = _engine(urm)
    norm = np.ones(70)
    bad = [lambda: eng.userknn_fit(6, 5), lambda: eng.userknn_fit(-1, 5), lambda: eng.userknn_fit(HI.RAW, 0),
           lambda: eng.userknn_fit(HI.RAW, L.ITEMKNN_MAX_TOPK + 1), lambda: eng.userknn_fit(HI.RAW, 5, shrink=-1.0),
           lambda: eng.userknn_fit(HI.SHRINK_ONLY, 5, shrink=0.0), lambda: eng.userknn_fit(HI.PRODUCT, 5, den_a=norm),
           lambda: eng.userknn_fit(HI.TANIMOTO, 5), lambda: eng.userknn_fit(HI.DICE, 5, den_a=np.full(70, np.inf)),
           lambda: eng.scores(np.arange(3)),      # no W yet
           lambda: eng.user_similarity(), lambda: eng.item_similarity()]
    for call in bad:
        with pytest.raises(L.GanmfError):
            call()
    eng.userknn_fit(HI.PRODUCT, 5, den_a=norm, den_b=norm)
    W = eng.user_similarity()
    ref = eng.scores(np.arange(70))

    def still_works():
        assert (eng.user_similarity() != W).nnz == 0 and np.array_equal(eng.scores(np.arange(70)), ref)

    with pytest.raises(L.GanmfError, match="user similarity"):      # the item entry while a user matrix is held
        eng.item_similarity()
    still_works()
    with pytest.raises(L.GanmfError, match="transposed"):
        eng.scores(np.arange(3), transposed=True)
    with pytest.raises(L.GanmfError, match="transposed"):
        eng.recommend(np.arange(3), 5, transposed=True)
    with pytest.raises(L.GanmfError, match="not finite"):
        eng.set_user_similarity(sps.csr_matrix(([np.nan], ([0], [1])), shape=(70, 70)))
    with pytest.raises(ValueError):
        eng.set_user_similarity(sps.identity(50, format="csr"))      # the item count, not the user count
    ip = np.zeros(51, dtype=np.int64)
    rc = eng.lib.ganmf_set_user_similarity(eng.h, ip.ctypes.data_as(C.POINTER(C.c_int64)), None, None, 50)
    assert rc == -1 and b"70 users" in L.load_library().ganmf_last_error()
    bad_ip = np.array([0] + [1] * 70, dtype=np.int64)
    col = np.array([70], dtype=np.int32)
    one = np.ones(1, dtype=np.float32)
    rc = eng.lib.ganmf_set_user_similarity(eng.h, bad_ip.ctypes.data_as(C.POINTER(C.c_int64)), col.ctypes.data_as(C.POINTER(C.c_int32)),
                                           one.ctypes.data_as(C.POINTER(C.c_float)), 70)
    assert rc == -1 and b"out of range" in L.load_library().ganmf_last_error()
    with pytest.raises(L.GanmfError):      # a fit refused for its arguments keeps the matrix the handle holds
        eng.userknn_fit(HI.RAW, 0)
    still_works()
    # an item matrix on the same handle replaces the user matrix, and the other way round
    eng.set_confidence(1, sps.csr_matrix(urm.T))
    eng.itemknn_fit(HI.RAW, 5)
    with pytest.raises(L.GanmfError, match="item similarity"):
        eng.user_similarity()
    assert eng.item_similarity().shape == (50, 50)
    item_scores = eng.scores(np.arange(70))
    np.testing.assert_array_equal(item_scores.astype(np.float64), HI.scores(urm, eng.item_similarity()))      # integers: exact
    eng.set_user_similarity(W)
    still_works()
    with pytest.raises(L.GanmfError, match="user similarity"):
        eng.item_similarity()
    # a missing side 0, a side 0 that is not canonical, a data-parallel handle, a handle of another model
    half = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM)
    half.set_confidence(1, sps.csr_matrix(urm.T))
    with pytest.raises(L.GanmfError, match="side 0"):
        half.userknn_fit(HI.RAW, 5)
    m = sps.csr_matrix(urm)
    at = m.indptr[np.flatnonzero(np.diff(m.indptr) >= 2)[0]]
    idx = m.indices.copy()
    idx[[at, at + 1]] = idx[[at + 1, at]]      # one user whose first two items descend
    half.set_confidence(0, sps.csr_matrix((m.data, idx, m.indptr), shape=m.shape))
    with pytest.raises(L.GanmfError, match="canonical"):
        half.userknn_fit(HI.RAW, 5)
    half.set_confidence(0, m)
    assert half.userknn_fit(HI.RAW, 5) > 0      # the same handle, once side 0 is right
    half.close()
    dp = Engine(70, 50, 1, 1, 1, model=L.MODEL_ITEMSIM, world_size=2, rank=0)      # a data-parallel handle
    dp.comm_init_local(7304)
    with pytest.raises(L.GanmfError, match="single-GPU"):
        dp.userknn_fit(HI.RAW, 5)
    with pytest.raises(L.GanmfError, match="single-GPU"):
        dp.set_user_similarity(W)
    dp.close()
    mf = Engine(70, 50, 2, 1, 1, model=L.MODEL_MF)
    with pytest.raises(L.GanmfError, match="ITEMSIM"):
        mf.userknn_fit(HI.RAW, 5)
    with pytest.raises(L.GanmfError, match="ITEMSIM"):
        mf.set_user_similarity(W)
    mf.close()
    still_works()
    eng.close()
