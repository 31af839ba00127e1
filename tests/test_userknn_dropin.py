"""UserKNNCFRecommender as a drop-in: the reference's import path, name, constants and signatures (KNN/UserKNNCFRecommender.py:18-61),
compared with the reference's own file where a reference tree is on sys.path; and the binding of the three library entries."""
import ast
import inspect
import os
import re

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_import_path_and_name():
    from KNN.UserKNNCFRecommender import UserKNNCFRecommender
    from ganmf_amd.UserKNN import UserKNNCFRecommender as Impl
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender
    from ganmf_amd.knn_model import NeighbourhoodCFRecommender
    assert UserKNNCFRecommender.__module__.split(".")[0] == "KNN"
    assert issubclass(UserKNNCFRecommender, Impl)
    assert UserKNNCFRecommender.RECOMMENDER_NAME == "UserKNNCFRecommender"
    assert UserKNNCFRecommender.FEATURE_WEIGHTING_VALUES == ["BM25", "TF-IDF", "none"]
    # one fit() for the two neighbourhood models, not a copy
    assert Impl.fit is ItemKNNCFRecommender.fit is NeighbourhoodCFRecommender.fit
    assert not issubclass(Impl, ItemKNNCFRecommender)


def test_signatures():
    from KNN.UserKNNCFRecommender import UserKNNCFRecommender
    init = inspect.signature(UserKNNCFRecommender.__init__)
    assert list(init.parameters)[:2] == ["self", "URM_train"]
    assert all(p.default is not inspect.Parameter.empty for p in list(init.parameters.values())[2:])
    fit = inspect.signature(UserKNNCFRecommender.fit)
    names = list(fit.parameters)
    assert names == ["self", "topK", "shrink", "similarity", "normalize", "feature_weighting", "similarity_args"]
    assert fit.parameters["similarity_args"].kind is inspect.Parameter.VAR_KEYWORD
    defaults = {n: fit.parameters[n].default for n in names[1:6]}
    assert defaults == dict(topK=50, shrink=100, similarity="cosine", normalize=True, feature_weighting="none")
    for method in ("recommend", "saveModel", "loadModel", "get_URM_train", "set_items_to_ignore", "_compute_item_score"):
        assert callable(getattr(UserKNNCFRecommender, method))
    assert isinstance(UserKNNCFRecommender.W_sparse, property)


def _reference_file():
    """KNN/UserKNNCFRecommender.py of a reference tree on sys.path (where KNN/__init__.py looks for the package's other modules), else
    None"""
    import sys
    for base in sys.path:
        path = os.path.join(base or ".", "KNN", "UserKNNCFRecommender.py")
        if os.path.exists(path) and not os.path.samefile(os.path.dirname(os.path.dirname(path)), ROOT):
            return path
    return None


def test_signatures_equal_the_reference_file_when_present():
    """the reference's class, read as text (it is not imported): name, constants, and the parameters and defaults of __init__ / fit"""
    from KNN.UserKNNCFRecommender import UserKNNCFRecommender
    path = _reference_file()
    if path is None:      # nothing to compare with: the pinned signature of test_signatures stands alone
        return
    cls = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "UserKNNCFRecommender"][0]
    consts = {t.id: ast.literal_eval(n.value) for n in cls.body if isinstance(n, ast.Assign) for t in n.targets}
    assert consts["RECOMMENDER_NAME"] == UserKNNCFRecommender.RECOMMENDER_NAME
    assert consts["FEATURE_WEIGHTING_VALUES"] == UserKNNCFRecommender.FEATURE_WEIGHTING_VALUES
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    ours = inspect.signature(UserKNNCFRecommender.fit)
    ref = fns["fit"].args
    assert [a.arg for a in ref.args] == list(ours.parameters)[:len(ref.args)]
    assert ref.kwarg.arg == "similarity_args"
    ref_defaults = dict(zip([a.arg for a in ref.args][-len(ref.defaults):], [ast.literal_eval(d) for d in ref.defaults]))
    assert ref_defaults == {n: ours.parameters[n].default for n in ref_defaults}
    assert [a.arg for a in fns["__init__"].args.args] == list(inspect.signature(UserKNNCFRecommender.__init__).parameters)[:2]


def test_constructor_holds_the_urm_and_reports_cold_users(capsys):
    from KNN.UserKNNCFRecommender import UserKNNCFRecommender
    urm = sps.random(12, 7, density=0.3, format="csr", dtype=np.float32, random_state=1).tolil()
    urm[4, :] = 0
    urm[9, :] = 0
    urm = sps.csr_matrix(urm)
    urm.eliminate_zeros()
    m = UserKNNCFRecommender(urm)
    assert (m.n_users, m.n_items) == (12, 7) and m.get_URM_train().shape == (12, 7)
    assert m.mode == "user" and m.score_contract == "mf" and m.mask_cold_users is False and m.honours_items_to_compute
    assert capsys.readouterr().out == ""
    UserKNNCFRecommender(urm, verbose=True)
    assert capsys.readouterr().out == "UserKNNCFRecommender: Detected 2 (16.67 %) cold users.\n"


def test_entries_are_declared_documented_and_bound():
    from ganmf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "ganmf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load_library()
    for name in ("ganmf_userknn_fit", "ganmf_userknn_get", "ganmf_set_user_similarity"):
        assert re.search(r"\bint %s\s*\(ganmf_handle\* h," % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, "%s is declared but not described in the header" % name
    fit_args = lambda n: re.search(r"int %s\s*\((.*?)\);" % n, code, flags=re.S).group(1).split(",")
    assert len(fit_args("ganmf_userknn_fit")) == len(fit_args("ganmf_itemknn_fit")) == 9
    assert lib.ganmf_userknn_fit.argtypes == lib.ganmf_itemknn_fit.argtypes
    assert lib.ganmf_userknn_get.argtypes == lib.ganmf_itemknn_get.argtypes
    assert lib.ganmf_set_user_similarity.argtypes == lib.ganmf_set_item_similarity.argtypes
