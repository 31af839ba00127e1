"""P3alphaRecommender and RP3betaRecommender without a device: the float64 restatement (tests/helpers_p3.py) against the reference's
own output (tests/golden/p3_tiny.npz, written by tools/make_p3_fixture.py, every case tie-free), and the classes' host logic -- the
min_rating / implicit step, what each fit uploads, the clamp, every ValueError, the modified URM used for scoring, persistence --
against helpers_p3.HelperEngine."""
import json
import os
import zipfile

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd import _lib as L
from ganmf_amd.P3 import P3alphaRecommender, RP3betaRecommender, transition_terms
from tests import helpers_p3 as H

CLASSES = {"P3alpha": P3alphaRecommender, "RP3beta": RP3betaRecommender}


@pytest.fixture(scope="module")
def tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, "p3_tiny.npz"))
    cases = json.loads(str(z["cases"]))
    return z, cases


def _model(urm, cls=P3alphaRecommender):
    model = cls(urm)
    model._make_engine = lambda: H.HelperEngine(model.n_users, model.n_items)
    return model


def _helper_fit(urm, case, **kw):
    data = H.apply_min_rating(urm, case.get("min_rating", 0), case.get("implicit", False))
    return data, H.fit(data, topK=case["topK"], alpha=case["alpha"], beta=case.get("beta"),
                       normalize_similarity=case.get("normalize_similarity", False), **kw)


def _assert_same(got, want):
    """two dense W: the same pattern, exactly (the fixture's cases are tie-free), the values within rtol 1e-6 (the fixture's went
    through float32)"""
    assert got.shape == want.shape
    np.testing.assert_array_equal(got != 0, want != 0)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_fixture_holds_every_case(tiny):
    z, cases = tiny
    assert z["urm"].shape == (40, 30) and set(np.unique(z["urm"])) <= {0, 1, 2, 3, 4, 5}
    assert not z["urm"][:, 11].any() and not z["urm"][7].any()
    assert [c["model"] for c in cases] == ["P3alpha"] * 5 + ["RP3beta"] * 2
    assert len(cases) == 7 and all("W_%d" % n in z.files for n in range(7))
    flat = [(c["model"], c["topK"], c["alpha"], c.get("beta"), bool(c.get("normalize_similarity", False))) for c in cases]
    for want in [("P3alpha", 5, 0.7, None, True), ("P3alpha", 3, 1.0, None, False), ("P3alpha", 29, 1.6, None, True),
                 ("P3alpha", 100, 0.3, None, False), ("RP3beta", 6, 0.8, 0.4, True), ("RP3beta", 4, 1.0, 1.2, False)]:
        assert want in flat
    filtered = [c for c in cases if c.get("min_rating", 0) > 0]
    assert len(filtered) == 1 and filtered[0]["min_rating"] == 3 and filtered[0]["implicit"] and filtered[0]["alpha"] == 0.7
    # the second selection has something to do in the fixture: some case keeps fewer entries than its rows selected
    urm = sps.csr_matrix(z["urm"])
    rs, pui, _ = H.transition_terms(urm, 0.7)
    assert H.select_rows(H.rows_sparse(rs, pui), 5).nnz > int((z["W_0"] != 0).sum())


def test_fixture_cases_are_tie_free(tiny):
    z, cases = tiny
    urm = sps.csr_matrix(z["urm"])
    for case in cases:
        _, a = _helper_fit(urm, case)
        _, b = _helper_fit(urm, case, larger_id=True)
        assert (a != b).nnz == 0, case


def test_restatement_equals_the_reference(tiny):
    z, cases = tiny
    urm = sps.csr_matrix(z["urm"])
    for n, case in enumerate(cases):
        _, W = _helper_fit(urm, case)
        _assert_same(W.toarray(), z["W_%d" % n])


def test_restatement_steps_on_a_hand_made_matrix():
    """3 users x 3 items, alpha = 1: u0 rated items 0 and 1 (2 and 6), u1 items 1 and 2 (1 and 1), u2 item 0"""
    urm = sps.csr_matrix(np.array([[2, 6, 0], [0, 1, 1], [5, 0, 0]], dtype=np.float32))
    rs, pui, cs = H.transition_terms(urm, 1.0, 1.0)
    np.testing.assert_allclose(rs, [0.5, 0.5, 1.0])
    np.testing.assert_allclose(cs, [0.5, 0.5, 1.0])
    np.testing.assert_allclose(pui.toarray(), np.array([[0.25, 0.75, 0], [0, 0.5, 0.5], [1, 0, 0]]).T)
    w = H.rows_dense(rs, pui)
    np.testing.assert_allclose(w, [[0, 0.375, 0], [0.125, 0, 0.25], [0, 0.5, 0]])
    np.testing.assert_allclose(H.rows_dense(rs, pui, cs), [[0, 0.1875, 0], [0.0625, 0, 0.25], [0, 0.25, 0]])
    R = H.select_rows(w, 1)
    np.testing.assert_allclose(R.toarray(), [[0, 0.375, 0], [0, 0, 0.25], [0, 0.5, 0]])
    np.testing.assert_allclose(H.normalize_rows(H.select_rows(w, 2)).toarray(), [[0, 1, 0], [1 / 3, 0, 2 / 3], [0, 1, 0]])
    np.testing.assert_allclose(H.select_columns(R, 1).toarray(), [[0, 0, 0], [0, 0, 0.25], [0, 0.5, 0]])      # column 1: 0.5 beats 0.375
    tied = sps.csr_matrix(np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.float32))
    assert H.select_rows(tied, 1).indices.tolist() == [1, 0, 0] and H.select_rows(tied, 1, larger_id=True).indices.tolist() == [2, 2, 1]
    assert H.select_columns(tied, 1).toarray().tolist() == [[0, 1, 1], [1, 0, 0], [0, 0, 0]]
    assert H.select_columns(tied, 1).dtype == np.float32


def test_class_fit_equals_the_reference_on_the_helper_engine(tiny):
    """both classes, driven through the float64 engine, reproduce the reference's W_sparse, and the scores come from the URM_train
    that fit() modified"""
    z, cases = tiny
    for n, case in enumerate(cases):
        args = dict(case)
        model = _model(sps.csr_matrix(z["urm"]), CLASSES[args.pop("model")])
        model.fit(**args)
        W = model.W_sparse
        assert sps.isspmatrix_csr(W) and W.dtype == np.float32 and W.shape == (30, 30)
        _assert_same(np.asarray(W.todense(), dtype=np.float64), z["W_%d" % n])
        data = H.apply_min_rating(sps.csr_matrix(z["urm"]), case.get("min_rating", 0), case.get("implicit", False))
        assert (model.URM_train != data).nnz == 0 and model._URM_eval is model.URM_train
        want = data.toarray().astype(np.float64).dot(model.engine.W.toarray())
        np.testing.assert_allclose(model._compute_item_score(np.arange(40)), want, rtol=2e-6, atol=1e-9)
        assert model.engine.mask_cold is False      # a user without ratings scores zeros, not -inf
        assert np.all(model._compute_item_score(np.array([7])) == 0)


@pytest.mark.parametrize("cls, alpha, beta", [(P3alphaRecommender, 1.0, None), (P3alphaRecommender, 0.6, None),
                                              (RP3betaRecommender, 1.0, 0.6), (RP3betaRecommender, 1.7, -0.3)])
def test_what_each_fit_uploads(tiny, cls, alpha, beta):
    z, _ = tiny
    urm = sps.csr_matrix(z["urm"])
    model = _model(urm, cls)
    kw = dict(topK=1000, alpha=alpha, normalize_similarity=True)
    if beta is not None:
        kw["beta"] = beta
    model.fit(**kw)
    eng = model.engine
    a = eng.fit_args
    assert a["topk"] == 30 and a["col_topk"] == 30 and a["normalize"] is True      # topK clamped to the item count
    rs, pui, cs = H.transition_terms(urm, alpha, beta)
    up = eng.conf_at_fit[1]
    assert up.dtype == np.float32 and a["row_scale"].dtype == np.float32
    assert np.array_equal(up.indptr, pui.indptr) and np.array_equal(up.indices, pui.indices)
    np.testing.assert_array_equal(up.data, pui.data.astype(np.float32))      # float64 terms, rounded to float32 once
    np.testing.assert_array_equal(a["row_scale"], rs.astype(np.float32))
    assert a["row_scale"][11] == 0      # the item nobody rated
    if beta is None:
        assert a["col_scale"] is None
    else:
        assert a["col_scale"].dtype == np.float32 and a["col_scale"][11] == 0
        np.testing.assert_array_equal(a["col_scale"], cs.astype(np.float32))
    dense = z["urm"].astype(np.float64)
    np.testing.assert_array_equal(eng.conf_at_fit[0].toarray(), dense)      # the scores read the ratings themselves
    np.testing.assert_array_equal(eng.conf[0].toarray(), dense)
    np.testing.assert_array_equal(eng.conf[1].toarray(), dense.T)           # side 1 restored after the fit


def test_min_rating_and_implicit_semantics(tiny):
    z, _ = tiny
    urm = sps.csr_matrix(z["urm"])
    plain = _model(urm)
    plain.fit(topK=5, alpha=0.7)
    alone = _model(urm)
    alone.fit(topK=5, alpha=0.7, implicit=True)      # implicit without min_rating > 0 does nothing
    assert (alone.URM_train != urm).nnz == 0 and (alone.W_sparse != plain.W_sparse).nnz == 0
    cut = _model(urm)
    before = cut.URM_train
    cut.fit(topK=5, alpha=0.7, min_rating=3)
    assert cut.URM_train is before      # modified in place
    assert cut.URM_train.data.min() == 3 and cut.URM_train.nnz == int((z["urm"] >= 3).sum())
    np.testing.assert_array_equal(cut.engine.conf[0].toarray(), np.where(z["urm"] >= 3, z["urm"], 0))
    ones = _model(urm)
    ones.fit(topK=5, alpha=0.7, min_rating=3, implicit=True)
    np.testing.assert_array_equal(ones.engine.conf[0].toarray(), (z["urm"] >= 3) * 1.0)
    assert ones.URM_train.dtype == np.float32 and (ones.W_sparse != cut.W_sparse).nnz != 0
    assert str(ones) == "P3alpha(alpha=0.7, min_rating=3, topk=5, implicit=True, normalize_similarity=False)"


def test_a_stored_zero_counts_in_the_degree(tiny):
    z, _ = tiny
    urm = sps.csr_matrix(z["urm"])
    model = _model(urm)
    at = model.URM_train.indptr[3]      # user 3's first stored rating becomes an explicit zero
    item = model.URM_train.indices[at]
    model.URM_train.data[at] = 0.0
    model.fit(topK=5, alpha=1.0)
    deg = np.bincount(urm.indices, minlength=30)
    assert model.engine.fit_args["row_scale"][item] == np.float32(1.0 / deg[item])      # the degree still counts the entry
    up = model.engine.conf_at_fit[1]
    assert up.nnz == urm.nnz and up[item, 3] == 0 and 3 in up.indices[up.indptr[item]:up.indptr[item + 1]]
    rs, pui, _ = transition_terms(model.URM_train, 1.0)
    rs64, pui64, _ = H.transition_terms(model.URM_train, 1.0)
    np.testing.assert_array_equal(rs, rs64.astype(np.float32))
    np.testing.assert_array_equal(pui.data, pui64.data.astype(np.float32))


def test_argument_errors_need_no_device(tiny):
    z, _ = tiny
    for cls in (P3alphaRecommender, RP3betaRecommender):
        model = _model(sps.csr_matrix(z["urm"]), cls)
        with pytest.raises(ValueError, match="topK"):
            model.fit(topK=0)
        for alpha in (0, -0.5, np.inf, np.nan):
            with pytest.raises(ValueError, match="alpha"):
                model.fit(alpha=alpha)
        if cls is RP3betaRecommender:
            for beta in (np.inf, np.nan):
                with pytest.raises(ValueError, match="beta"):
                    model.fit(beta=beta)
        assert model.engine is None
        with pytest.raises(RuntimeError):
            model.W_sparse
        with pytest.raises(RuntimeError):
            model._compute_item_score(np.arange(3))
        for value in (-1.0, np.inf, np.nan):
            bad = _model(sps.csr_matrix(z["urm"]), cls)
            bad.URM_train.data[0] = value
            with pytest.raises(ValueError, match="ratings"):
                bad.fit()
            assert bad.engine is None
    with pytest.raises(TypeError):
        _model(sps.csr_matrix(z["urm"])).fit(beta=0.5)


def test_topk_above_the_device_limit_is_refused_only_when_it_survives_the_clamp():
    wide = sps.random(5, L.ITEMKNN_MAX_TOPK + 6, density=0.5, format="csr", dtype=np.float32, random_state=3)
    model = _model(wide)
    with pytest.raises(ValueError, match="at most"):
        model.fit(topK=L.ITEMKNN_MAX_TOPK + 1)
    assert model.engine is None
    model.fit(topK=L.ITEMKNN_MAX_TOPK)
    assert model.engine.fit_args["topk"] == L.ITEMKNN_MAX_TOPK
    small = _model(sps.random(5, 9, density=0.5, format="csr", dtype=np.float32, random_state=3), RP3betaRecommender)
    small.fit(topK=10 ** 6)
    assert small.engine.fit_args["topk"] == 9 and small.engine.fit_args["col_topk"] == 9 and small.topK == 10 ** 6


def test_items_to_compute_and_candidate_hooks(tiny):
    z, _ = tiny
    model = _model(sps.csr_matrix(z["urm"]), RP3betaRecommender)
    model.fit(topK=5)
    s = model._compute_item_score(np.arange(40), items_to_compute=[2, 3])
    assert np.all(np.isneginf(np.delete(s, [2, 3], axis=1))) and np.all(np.isfinite(s[:, [2, 3]]))
    assert model.honours_items_to_compute
    cand = sps.csr_matrix(np.ones((40, 30)))
    assert model.evaluate_candidates_on_device(1, None, None, cand, np.arange(3), [5], None, None) is None
    assert model._device_ranking_args(np.arange(3), [5], 256, candidates_csr=cand) is None
    assert model._device_ranking_args(np.arange(3), [5], 256) is not None
    with pytest.raises(NotImplementedError):
        model.prediction_similarity()
    with pytest.raises(NotImplementedError):
        model.recommend_candidates(np.arange(3), cand, 5)


@pytest.mark.parametrize("cls", [P3alphaRecommender, RP3betaRecommender])
def test_save_and_load_use_the_reference_layout(tiny, tmp_path, cls):
    z, _ = tiny
    urm = sps.csr_matrix(z["urm"])
    model = _model(urm, cls)
    model.fit(topK=6, alpha=0.8)
    model.saveModel(str(tmp_path), file_name="p3")
    with zipfile.ZipFile(os.path.join(str(tmp_path), "p3.zip")) as zf:
        assert sorted(zf.namelist()) == ["W_sparse.npz", "__DataIO_attribute_to_file_name.json", "__DataIO_attribute_to_type_dict.json"]
        assert json.loads(zf.read("__DataIO_attribute_to_type_dict.json").decode()) == {"W_sparse": "sps.spmatrix"}
        assert json.loads(zf.read("__DataIO_attribute_to_file_name.json").decode()) == {"W_sparse": "W_sparse.npz"}
    model.saveModel(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), cls.RECOMMENDER_NAME + ".zip"))
    other = _model(urm, cls)
    other.loadModel(str(tmp_path), file_name="p3")
    a, b = model.W_sparse, other.W_sparse
    assert (a != b).nnz == 0 and b.dtype == np.float32
    np.testing.assert_allclose(other._compute_item_score(np.arange(40)), model._compute_item_score(np.arange(40)), rtol=1e-6)
    wrong = _model(sps.csr_matrix(z["urm"][:, :20]), cls)
    with pytest.raises(ValueError, match="items"):
        wrong.loadModel(str(tmp_path), file_name="p3")


def test_trial_log_fixture(golden_dir):
    doc = json.load(open(os.path.join(golden_dir, "p3_trial_logs_ml1m.json")))
    trials = doc["trials"]
    assert doc["metric"] == "MAP" and doc["at"] == 5
    assert [t["role"] for t in trials] == ["trial", "trial", "trial", "best"]
    for t in trials:
        assert set(t["params"]) == {"topK", "alpha", "normalize_similarity"}
        assert all(0 < t[k] < 1 for k in ("logged", "replayed", "restated64", "restated32"))
    latitude = max(abs(t[k] - t["replayed"]) for t in trials for k in ("logged", "restated64", "restated32"))
    assert doc["latitude"] == latitude
    assert 4 * doc["latitude"] + 1e-6 < 1.0 / (2 * 6040)      # the device's bound still catches one user's list going wrong
