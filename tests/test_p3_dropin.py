"""P3alphaRecommender and RP3betaRecommender as drop-ins: the reference's import paths, names and signatures
(GraphBased/P3alphaRecommender.py:19-33, GraphBased/RP3betaRecommender.py:16-30), and the binding of ganmf_p3_fit."""
import inspect

import numpy as np
import scipy.sparse as sps


def test_import_paths_and_names():
    from GraphBased.P3alphaRecommender import P3alphaRecommender
    from GraphBased.RP3betaRecommender import RP3betaRecommender
    from ganmf_amd import P3
    assert P3alphaRecommender.__module__ == "GraphBased.P3alphaRecommender" and issubclass(P3alphaRecommender, P3.P3alphaRecommender)
    assert RP3betaRecommender.__module__ == "GraphBased.RP3betaRecommender" and issubclass(RP3betaRecommender, P3.RP3betaRecommender)
    assert P3alphaRecommender.RECOMMENDER_NAME == "P3alphaRecommender"
    assert RP3betaRecommender.RECOMMENDER_NAME == "RP3betaRecommender"


def test_signatures():
    from GraphBased.P3alphaRecommender import P3alphaRecommender
    from GraphBased.RP3betaRecommender import RP3betaRecommender
    want = {P3alphaRecommender: [("topK", 100), ("alpha", 1.), ("min_rating", 0), ("implicit", False), ("normalize_similarity", False)],
            RP3betaRecommender: [("alpha", 1.), ("beta", 0.6), ("min_rating", 0), ("topK", 100), ("implicit", False),
                                 ("normalize_similarity", True)]}
    for cls, args in want.items():
        init = inspect.signature(cls.__init__)
        assert list(init.parameters) == ["self", "URM_train", "device", "verbose"]
        assert init.parameters["device"].default == 0 and init.parameters["verbose"].default is False
        fit = inspect.signature(cls.fit)
        assert [(n, p.default) for n, p in list(fit.parameters.items())[1:]] == args
        for method in ("recommend", "saveModel", "loadModel", "get_URM_train", "set_items_to_ignore", "_compute_item_score"):
            assert callable(getattr(cls, method))
        assert isinstance(cls.W_sparse, property)


def test_constructor_holds_the_urm_and_str_is_the_reference_s():
    from GraphBased.P3alphaRecommender import P3alphaRecommender
    from GraphBased.RP3betaRecommender import RP3betaRecommender
    from tests import helpers_p3 as H
    urm = sps.random(12, 7, density=0.3, format="csr", dtype=np.float32, random_state=1)
    for cls in (P3alphaRecommender, RP3betaRecommender):
        m = cls(urm)
        assert (m.n_users, m.n_items) == (12, 7) and m.get_URM_train().shape == (12, 7)
        assert m.mode == "user" and m.score_contract == "mf" and m.mask_cold_users is False and m.honours_items_to_compute is True
        m._make_engine = lambda: H.HelperEngine(12, 7)
        m.fit(topK=3, alpha=0.5)
    assert str(m) == "RP3beta(alpha=0.5, beta=0.6, min_rating=0, topk=3, implicit=False, normalize_similarity=True)"


def test_the_entry_is_declared_and_bound():
    import os
    import re
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ganmf_hip.h")).read()
    assert re.search(r"int ganmf_p3_fit\(ganmf_handle\* h, int32_t topk, int32_t col_topk, int normalize,\s*const float\* row_scale, "
                     r"const float\* col_scale,\s*int64_t\* nnz\);", text)
    assert "ganmf_p3_fit" in L.SYMBOLS
    assert list(inspect.signature(Engine.p3_fit).parameters) == ["self", "topk", "row_scale", "col_scale", "normalize", "col_topk"]
    assert int(re.search(r"#define GANMF_ABI_VERSION (\d+)", text).group(1)) == L.ABI_VERSION == 2
    # the new profile classes stand at the end of the timer enum: every earlier index stays
    base = open(os.path.join(root, "ganmf_amd", "csrc", "lib", "base.inc")).read()
    tags = re.search(r"enum Tag : int \{(.*?)\};", base, re.S).group(1).replace("\n", " ").split(",")
    assert [t.strip() for t in tags][-7:] == ["T_KNN_FIT", "T_KNN_PACK", "T_KNN_SCORE", "T_P3_ROWS", "T_P3_NORMALIZE", "T_P3_COLUMNS", "T_COUNT"]
