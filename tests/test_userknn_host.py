"""UserKNNCFRecommender without a device: the class's host logic -- what each similarity uploads (per-USER denominators, ones on side
0 for the binarising similarities and URM_train's values back before anything is scored), the clamps, every ValueError, the weighted
URM used for scoring, persistence -- against helpers_userknn.HelperEngine, whose fit is helpers_itemknn's on the transposed matrix."""
import json
import os
import zipfile

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd import _lib as L
from ganmf_amd.UserKNN import UserKNNCFRecommender
from ganmf_amd.knn_model import TF_IDF, okapi_BM_25
from tests import helpers_itemknn as HI
from tests import helpers_userknn as H


@pytest.fixture(scope="module")
def urm(golden_dir):
    """the 40 x 30 matrix of the item-KNN fixture (ratings 1..5, user 7 without ratings)"""
    z = np.load(os.path.join(golden_dir, "itemknn_tiny.npz"))
    return sps.csr_matrix(z["urm"].astype(np.float32))


def _model(urm):
    model = UserKNNCFRecommender(urm)
    model._make_engine = lambda: H.HelperEngine(model.n_users, model.n_items)
    return model


def test_helper_fit_is_the_item_fit_of_the_transpose(urm):
    for kw in (dict(similarity="cosine", shrink=3), dict(similarity="tversky", shrink=1, tversky_alpha=0.4, tversky_beta=1.2),
               dict(similarity="cosine", normalize=False, shrink=0)):
        W = H.fit(urm, topK=6, **kw)
        assert W.shape == (40, 40) and (W != HI.fit(urm.T.tocsr(), topK=6, **kw)).nnz == 0
        assert np.diff(W.tocsc().indptr).max() == 6 and np.diff(W.indptr).max() > 6      # bounded by column, not by row
        assert W[7].nnz == 0 and W[:, 7].nnz == 0      # the user without ratings
    W = H.fit(urm, topK=6, shrink=0)
    np.testing.assert_allclose(H.scores(urm, W), W.toarray().dot(urm.toarray().astype(np.float64)), rtol=1e-13)      # (summation order)
    np.testing.assert_array_equal(H.scores(urm, W, [3, 3, 0]), H.scores(urm, W)[[3, 3, 0]])
    np.testing.assert_array_equal(H.terms(urm, W), (W.toarray() != 0).astype(float).dot((urm.toarray() != 0).astype(float)))


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
def test_what_each_similarity_uploads(urm, similarity, normalize, shrink, kind, binary):
    model = _model(urm)
    extra = dict(asymmetric_alpha=0.3, tversky_alpha=0.6, tversky_beta=1.4)
    model.fit(topK=1000, shrink=shrink, similarity=similarity, normalize=normalize, **extra)
    eng = model.engine
    a = eng.fit_args
    assert a["kind"] == kind and a["topk"] == 40 and a["shrink"] == shrink      # topK clamped to the USER count
    dense = urm.toarray().astype(np.float64)
    seen_by_fit = np.asarray(eng.conf_at_fit[0].todense())
    np.testing.assert_array_equal(seen_by_fit, (dense != 0) * 1.0 if binary else dense)      # the fit reads side 0
    np.testing.assert_array_equal(np.asarray(eng.conf[0].todense()), dense)      # ... which is back at the ratings before any score
    np.testing.assert_array_equal(np.asarray(eng.conf[1].todense()), dense.T)
    sq = (dense * dense).sum(axis=1)      # per user
    if binary:
        np.testing.assert_array_equal(a["den_a"], (dense != 0).sum(axis=1))
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
    assert all(v is None or len(v) == 40 for v in (a["den_a"], a["den_b"]))
    assert eng.mask_cold is False      # a user without ratings scores zeros, not -inf
    # the class's W and scores are the restatement's
    W = model.W_sparse
    assert sps.isspmatrix_csr(W) and W.dtype == np.float32 and W.shape == (40, 40)
    want = H.fit(urm, topK=1000, shrink=shrink, similarity=similarity, normalize=normalize, **extra)
    np.testing.assert_allclose(W.toarray(), want.toarray(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(model._compute_item_score(np.arange(40)), H.scores(urm, eng.W), rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("weighting", ["BM25", "TF-IDF"])
def test_feature_weighting_replaces_urm_train(urm, weighting):
    model = _model(urm)
    model.fit(topK=5, shrink=1, feature_weighting=weighting)
    fn = okapi_BM_25 if weighting == "BM25" else TF_IDF
    weighted = sps.csr_matrix(fn(urm.astype(np.float32).T).T)      # (UserKNNCFRecommender.py:48-56: the same transposes as the item class)
    np.testing.assert_allclose(model.URM_train.toarray(), weighted.toarray(), rtol=1e-6, atol=1e-12)
    w32 = weighted.astype(np.float32).toarray().astype(np.float64)
    np.testing.assert_array_equal(np.asarray(model.engine.conf[0].todense()), w32)
    np.testing.assert_allclose(model.engine.fit_args["den_a"], np.sqrt((w32 * w32).sum(axis=1)), rtol=1e-14)
    want = H.fit(sps.csr_matrix(w32), topK=5, shrink=1)
    np.testing.assert_allclose(model.W_sparse.toarray(), want.toarray(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(model._compute_item_score(np.arange(40)), H.scores(sps.csr_matrix(w32), model.engine.W), rtol=2e-6, atol=1e-9)


def test_argument_errors_need_no_device(urm):
    model = _model(urm)
    for bad in ("adjusted", "pearson", "euclidean"):
        with pytest.raises(ValueError, match="not built"):
            model.fit(similarity=bad)
    with pytest.raises(ValueError, match="not recognized"):
        model.fit(similarity="manhattan")
    with pytest.raises(ValueError, match="feature_weighting"):
        model.fit(feature_weighting="bm25")
    with pytest.raises(ValueError, match="row_weights"):
        model.fit(row_weights=np.ones(30))
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


def test_topk_is_clamped_to_the_users_and_refused_above_the_device_limit():
    tall = sps.random(L.ITEMKNN_MAX_TOPK + 6, 5, density=0.5, format="csr", dtype=np.float32, random_state=3)
    model = _model(tall)
    with pytest.raises(ValueError, match="at most"):
        model.fit(topK=L.ITEMKNN_MAX_TOPK + 1)
    model.fit(topK=L.ITEMKNN_MAX_TOPK)
    assert model.engine.fit_args["topk"] == L.ITEMKNN_MAX_TOPK
    small = _model(sps.random(9, 2000, density=0.5, format="csr", dtype=np.float32, random_state=3))
    small.fit(topK=10 ** 6)
    assert small.engine.fit_args["topk"] == 9      # the users, not the 2000 items


def test_items_to_compute_and_candidate_hooks(urm):
    model = _model(urm)
    model.fit(topK=5, shrink=0)
    s = model._compute_item_score(np.arange(40), items_to_compute=[2, 3])
    assert np.all(np.isneginf(np.delete(s, [2, 3], axis=1))) and np.all(np.isfinite(s[:, [2, 3]]))
    assert np.all(model._compute_item_score(np.array([7])) == 0)      # the user without ratings is nobody's neighbour
    cand = sps.csr_matrix(np.ones((40, 30)))
    assert model.evaluate_candidates_on_device(1, None, None, cand, np.arange(3), [5], None, None) is None
    assert model._device_ranking_args(np.arange(3), [5], 256, candidates_csr=cand) is None
    assert model._device_ranking_args(np.arange(3), [5], 256) is not None
    with pytest.raises(NotImplementedError):
        model.prediction_similarity()
    with pytest.raises(NotImplementedError):
        model.recommend_candidates(np.arange(3), cand, 5)


def test_save_and_load_use_the_reference_layout(urm, tmp_path):
    model = _model(urm)
    model.fit(topK=6, shrink=1, similarity="dice")
    model.saveModel(str(tmp_path), file_name="knn")
    with zipfile.ZipFile(os.path.join(str(tmp_path), "knn.zip")) as zf:
        assert sorted(zf.namelist()) == ["W_sparse.npz", "__DataIO_attribute_to_file_name.json", "__DataIO_attribute_to_type_dict.json"]
        assert json.loads(zf.read("__DataIO_attribute_to_type_dict.json").decode()) == {"W_sparse": "sps.spmatrix"}
        assert json.loads(zf.read("__DataIO_attribute_to_file_name.json").decode()) == {"W_sparse": "W_sparse.npz"}
        import io
        assert sps.load_npz(io.BytesIO(zf.read("W_sparse.npz"))).shape == (40, 40)
    model.saveModel(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "UserKNNCFRecommender.zip"))
    other = _model(urm)
    other.loadModel(str(tmp_path), file_name="knn")
    a, b = model.W_sparse, other.W_sparse
    assert (a != b).nnz == 0 and b.dtype == np.float32 and b.shape == (40, 40)
    np.testing.assert_allclose(other._compute_item_score(np.arange(40)), model._compute_item_score(np.arange(40)), rtol=1e-6)
    wrong = _model(urm[:20])      # the same items, half the users
    with pytest.raises(ValueError, match="users"):
        wrong.loadModel(str(tmp_path), file_name="knn")
