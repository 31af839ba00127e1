"""ItemKNNCFRecommender as a drop-in: the reference's import path, name, constants and signatures
(KNN/ItemKNNCFRecommender.py:18-54)."""
import inspect

import numpy as np
import scipy.sparse as sps


def test_import_path_and_name():
    from KNN.ItemKNNCFRecommender import ItemKNNCFRecommender
    from ganmf_amd.ItemKNN import ItemKNNCFRecommender as Impl
    assert ItemKNNCFRecommender.__module__.split(".")[0] == "KNN"
    assert issubclass(ItemKNNCFRecommender, Impl)
    assert ItemKNNCFRecommender.RECOMMENDER_NAME == "ItemKNNCFRecommender"
    assert ItemKNNCFRecommender.FEATURE_WEIGHTING_VALUES == ["BM25", "TF-IDF", "none"]


def test_signatures():
    from KNN.ItemKNNCFRecommender import ItemKNNCFRecommender
    init = inspect.signature(ItemKNNCFRecommender.__init__)
    assert list(init.parameters)[:2] == ["self", "URM_train"]
    assert all(p.default is not inspect.Parameter.empty for p in list(init.parameters.values())[2:])
    fit = inspect.signature(ItemKNNCFRecommender.fit)
    names = list(fit.parameters)
    assert names == ["self", "topK", "shrink", "similarity", "normalize", "feature_weighting", "similarity_args"]
    assert fit.parameters["similarity_args"].kind is inspect.Parameter.VAR_KEYWORD
    defaults = {n: fit.parameters[n].default for n in names[1:6]}
    assert defaults == dict(topK=50, shrink=100, similarity="cosine", normalize=True, feature_weighting="none")
    for method in ("recommend", "saveModel", "loadModel", "get_URM_train", "set_items_to_ignore", "_compute_item_score"):
        assert callable(getattr(ItemKNNCFRecommender, method))
    assert isinstance(ItemKNNCFRecommender.W_sparse, property)


def test_constructor_holds_the_urm():
    from KNN.ItemKNNCFRecommender import ItemKNNCFRecommender
    urm = sps.random(12, 7, density=0.3, format="csr", dtype=np.float32, random_state=1)
    m = ItemKNNCFRecommender(urm)
    assert (m.n_users, m.n_items) == (12, 7) and m.get_URM_train().shape == (12, 7)
    assert m.mode == "user" and m.score_contract == "mf" and m.mask_cold_users is False


def test_constants_match_the_header():
    import os
    import re
    from ganmf_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ganmf_hip.h")).read()
    assert int(re.search(r"#define GANMF_ITEMKNN_MAX_TOPK (\d+)", text).group(1)) == L.ITEMKNN_MAX_TOPK
    assert int(re.search(r"GANMF_MODEL_ITEMSIM = (\d+)", text).group(1)) == L.MODEL_ITEMSIM
    for name in ("PRODUCT", "TANIMOTO", "DICE", "TVERSKY", "SHRINK_ONLY", "RAW"):
        assert int(re.search(r"GANMF_ITEMKNN_%s = (\d+)" % name, text).group(1)) == getattr(L, "ITEMKNN_" + name)
