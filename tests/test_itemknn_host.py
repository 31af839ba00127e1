"""ItemKNNCFRecommender without a device: the float64 restatement (tests/helpers_itemknn.py) against the reference's own output
(tests/golden/itemknn_tiny.npz, written by tools/make_itemknn_fixture.py), and the class's host logic -- what each similarity
uploads, the clamps, every ValueError, the weighted URM used for scoring, persistence -- against helpers_itemknn.HelperEngine."""
import json
import os
import zipfile

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd import _lib as L
from ganmf_amd.ItemKNN import TF_IDF, ItemKNNCFRecommender, okapi_BM_25
from tests import helpers_itemknn as H


@pytest.fixture(scope="module")
def tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, "itemknn_tiny.npz"))
    cases = json.loads(str(z["cases"]))
    return z, cases


def _model(urm):
    model = ItemKNNCFRecommender(urm)
    model._make_engine = lambda: H.HelperEngine(model.n_users, model.n_items)
    return model


def _fit_args(case):
    args = dict(case)
    return args.pop("feature_weighting", "none"), args


def _same_up_to_ties(got, want, sim=None):
    """two dense W: equal, or differing only in WHICH of several exactly tied neighbours a column kept (the reference's
    argpartition keeps an arbitrary one, the project the smaller id): the sorted values of every column agree"""
    assert got.shape == want.shape
    for i in range(got.shape[1]):
        a, b = np.sort(got[:, i])[::-1], np.sort(want[:, i])[::-1]
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=0, err_msg="column %d" % i)      # (the fixture's W went through float32)
        moved = np.flatnonzero((got[:, i] != 0) != (want[:, i] != 0))
        if len(moved) and sim is not None:      # every swapped neighbour sits at the column's smallest kept value
            cut = b[b != 0].min()
            np.testing.assert_allclose(sim[moved, i], cut, rtol=1e-6)


def test_fixture_holds_every_kind_and_both_weightings(tiny):
    z, cases = tiny
    assert z["urm"].shape == (40, 30) and set(np.unique(z["urm"])) <= {0, 1, 2, 3, 4, 5}
    assert {c["similarity"] for c in cases} >= {"cosine", "asymmetric", "jaccard", "tanimoto", "dice", "tversky"}
    assert {c.get("feature_weighting", "none") for c in cases} == {"none", "BM25", "TF-IDF"}
    assert any(not c["normalize"] and c["shrink"] == 0 for c in cases) and any(not c["normalize"] and c["shrink"] > 0 for c in cases)


def test_restatement_equals_the_reference(tiny):
    z, cases = tiny
    for n, case in enumerate(cases):
        weighting, args = _fit_args(case)
        urm = sps.csr_matrix(z["urm"]) if weighting == "none" else sps.csr_matrix(z["weighted_%d" % n])
        topK = args.pop("topK")
        shrink = args.pop("shrink")
        kind, X, p0, p1, den_a, den_b = H.host_plan(urm, args.pop("similarity"), args.pop("normalize"), shrink, **args)
        sim = H.similarity_dense(X, kind, shrink, p0, p1, den_a, den_b)
        got = np.asarray(H.w_sparse(sim, topK).todense())
        _same_up_to_ties(got, z["W_%d" % n], sim)


def test_feature_weightings_equal_the_reference(tiny):
    z, cases = tiny
    urm = sps.csr_matrix(z["urm"])
    for n, case in enumerate(cases):
        weighting = case.get("feature_weighting", "none")
        if weighting == "none":
            continue
        fn = okapi_BM_25 if weighting == "BM25" else TF_IDF
        got = np.asarray(fn(urm.astype(np.float32).T).T.todense())
        np.testing.assert_allclose(got, z["weighted_%d" % n], rtol=1e-6, atol=1e-12)


def test_class_fit_equals_the_reference_on_the_helper_engine(tiny):
    """the class's plan (kind, binarisation, denominators, clamp, weighting) driven through the float64 engine reproduces the
    reference's W_sparse, and the scores come from the (weighted) URM_train"""
    z, cases = tiny
    for n, case in enumerate(cases):
        weighting, args = _fit_args(case)
        model = _model(sps.csr_matrix(z["urm"]))
        model.fit(feature_weighting=weighting, **args)
        W = model.W_sparse
        assert sps.isspmatrix_csr(W) and W.dtype == np.float32 and W.shape == (30, 30)
        _same_up_to_ties(np.asarray(W.todense(), dtype=np.float64), z["W_%d" % n])
        users = np.arange(40)
        base = z["urm"] if weighting == "none" else z["weighted_%d" % n]
        want = base.astype(np.float64).dot(np.asarray(model.engine.W.todense()))
        np.testing.assert_allclose(model._compute_item_score(users), want, rtol=2e-6, atol=1e-9)
        if weighting != "none":
            np.testing.assert_allclose(np.asarray(model.URM_train.todense()), z["weighted_%d" % n], rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("similarity, normalize, shrink, kind, binary", [
    ("cosine", True, 7, L.ITEMKNN_PRODUCT, False),
    ("asymmetric", True, 0, L.ITEMKNN_PRODUCT, False),
    ("cosine", False, 7, L.ITEMKNN_SHRINK_ONLY, False),
    ("cosine", False, 0, L.ITEMKNN_RAW, False),
    ("asymmetric", False, 0, L.ITEMKNN_RAW, False),
    ("jaccard", True, 2, L.ITEMKNN_TANIMOTO, True),
    ("tanimoto", False, 2, L.ITEMKNN_TANIMOTO, True),
    ("dice", True, 2, L.ITEMKNN_DICE, True),
    ("tversky", True, 2, L.ITEMKNN_TVERSKY, True),
])
def test_what_each_similarity_uploads(tiny, similarity, normalize, shrink, kind, binary):
    z, _ = tiny
    urm = sps.csr_matrix(z["urm"])
    model = _model(urm)
    model.fit(topK=1000, shrink=shrink, similarity=similarity, normalize=normalize, asymmetric_alpha=0.3, tversky_alpha=0.6,
              tversky_beta=1.4)
    eng = model.engine
    a = eng.fit_args
    assert a["kind"] == kind and a["topk"] == 30 and a["shrink"] == shrink      # topK clamped to the item count
    seen_by_fit = np.asarray(eng.conf_at_fit[1].todense())
    dense = z["urm"].astype(np.float64)
    np.testing.assert_array_equal(seen_by_fit, ((dense != 0) * 1.0 if binary else dense).T)
    np.testing.assert_array_equal(np.asarray(eng.conf[0].todense()), dense)      # the scores always read the ratings themselves
    np.testing.assert_array_equal(np.asarray(eng.conf[1].todense()), dense.T)
    sq = (dense * dense).sum(axis=0)
    if binary:
        np.testing.assert_array_equal(a["den_a"], (dense != 0).sum(axis=0))
        assert a["den_b"] is None
        if similarity == "tversky":
            assert (a["p0"], a["p1"]) == (0.6, 1.4)
    elif kind == L.ITEMKNN_PRODUCT and similarity == "asymmetric":
        np.testing.assert_allclose(a["den_a"], np.sqrt(sq) ** 0.6, rtol=1e-14)
        np.testing.assert_allclose(a["den_b"], np.sqrt(sq) ** 1.4, rtol=1e-14)
    elif kind == L.ITEMKNN_PRODUCT:
        np.testing.assert_allclose(a["den_a"], np.sqrt(sq), rtol=1e-14)
        np.testing.assert_allclose(a["den_b"], np.sqrt(sq), rtol=1e-14)
    else:
        assert a["den_a"] is None and a["den_b"] is None
    assert eng.mask_cold is False      # a user without ratings scores zeros, not -inf


def test_argument_errors_need_no_device(tiny):
    z, _ = tiny
    model = _model(sps.csr_matrix(z["urm"]))
    for bad in ("adjusted", "pearson", "euclidean"):
        with pytest.raises(ValueError, match="not built"):
            model.fit(similarity=bad)
    with pytest.raises(ValueError, match="not recognized"):
        model.fit(similarity="manhattan")
    with pytest.raises(ValueError, match="feature_weighting"):
        model.fit(feature_weighting="bm25")
    with pytest.raises(ValueError, match="row_weights"):
        model.fit(row_weights=np.ones(40))
    with pytest.raises(ValueError, match="topK"):
        model.fit(topK=0)
    with pytest.raises(ValueError, match="shrink"):
        model.fit(shrink=-1)
    with pytest.raises(TypeError):
        model.fit(alpha=0.5)
    assert model.engine is None
    with pytest.raises(RuntimeError):
        model.W_sparse
    with pytest.raises(RuntimeError):
        model._compute_item_score(np.arange(3))


def test_topk_above_the_device_limit_is_refused_only_when_it_survives_the_clamp():
    wide = sps.random(5, L.ITEMKNN_MAX_TOPK + 6, density=0.5, format="csr", dtype=np.float32, random_state=3)
    model = _model(wide)
    with pytest.raises(ValueError, match="at most"):
        model.fit(topK=L.ITEMKNN_MAX_TOPK + 1)
    model.fit(topK=L.ITEMKNN_MAX_TOPK)
    assert model.engine.fit_args["topk"] == L.ITEMKNN_MAX_TOPK
    small = _model(sps.random(5, 9, density=0.5, format="csr", dtype=np.float32, random_state=3))
    small.fit(topK=10 ** 6)
    assert small.engine.fit_args["topk"] == 9


def test_items_to_compute_and_candidate_hooks(tiny):
    z, _ = tiny
    model = _model(sps.csr_matrix(z["urm"]))
    model.fit(topK=5, shrink=0)
    s = model._compute_item_score(np.arange(40), items_to_compute=[2, 3])
    assert np.all(np.isneginf(np.delete(s, [2, 3], axis=1))) and np.all(np.isfinite(s[:, [2, 3]]))
    assert np.all(model._compute_item_score(np.array([7])) == 0)      # the user without ratings
    assert model.honours_items_to_compute
    cand = sps.csr_matrix(np.ones((40, 30)))
    assert model.evaluate_candidates_on_device(1, None, None, cand, np.arange(3), [5], None, None) is None
    assert model._device_ranking_args(np.arange(3), [5], 256, candidates_csr=cand) is None
    assert model._device_ranking_args(np.arange(3), [5], 256) is not None
    with pytest.raises(NotImplementedError):
        model.prediction_similarity()
    with pytest.raises(NotImplementedError):
        model.recommend_candidates(np.arange(3), cand, 5)


def test_save_and_load_use_the_reference_layout(tiny, tmp_path):
    z, _ = tiny
    urm = sps.csr_matrix(z["urm"])
    model = _model(urm)
    model.fit(topK=6, shrink=1, similarity="dice")
    model.saveModel(str(tmp_path), file_name="knn")
    with zipfile.ZipFile(os.path.join(str(tmp_path), "knn.zip")) as zf:
        assert sorted(zf.namelist()) == ["W_sparse.npz", "__DataIO_attribute_to_file_name.json", "__DataIO_attribute_to_type_dict.json"]
        assert json.loads(zf.read("__DataIO_attribute_to_type_dict.json").decode()) == {"W_sparse": "sps.spmatrix"}
        assert json.loads(zf.read("__DataIO_attribute_to_file_name.json").decode()) == {"W_sparse": "W_sparse.npz"}
    model.saveModel(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "ItemKNNCFRecommender.zip"))
    other = _model(urm)
    other.loadModel(str(tmp_path), file_name="knn")
    a, b = model.W_sparse, other.W_sparse
    assert (a != b).nnz == 0 and b.dtype == np.float32
    # (the helper engine keeps its own W in float64 and a loaded one as float32 says: equal to float32)
    np.testing.assert_allclose(other._compute_item_score(np.arange(40)), model._compute_item_score(np.arange(40)), rtol=1e-6)
    wrong = _model(sps.csr_matrix(z["urm"][:, :20]))
    with pytest.raises(ValueError, match="items"):
        wrong.loadModel(str(tmp_path), file_name="knn")


def test_trial_log_fixture(golden_dir):
    doc = json.load(open(os.path.join(golden_dir, "itemknn_trial_logs_ml1m.json")))
    trials = doc["trials"]
    assert doc["metric"] == "MAP" and doc["at"] == 5
    for kind in ("cosine", "asymmetric", "jaccard", "dice", "tversky"):
        rows = [t for t in trials if t["kind"] == kind]
        assert [t["role"] for t in rows] == ["trial", "trial", "trial", "best"]
        assert all(t["params"]["similarity"] == kind and t["logged"] is not None and 0 < t["replayed"] < 1 for t in rows)
    spread = max(abs(t["logged"] - t["replayed"]) for t in trials if t["params"]["normalize"])
    assert 0 < spread < 1e-3      # two implementations of the reference agree to tie-breaking and float32
