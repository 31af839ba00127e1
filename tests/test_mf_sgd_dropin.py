"""The SGD matrix factorisations as drop-ins: the reference's import path, names and signatures
(MatrixFactorization/Cython/MatrixFactorization_Cython.py:19-245), the import sequence with a reference tree behind the repository, and
the binding of the ganmf_mf_sgd_* entries."""
import inspect
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {"_MatrixFactorization_Cython": "MatrixFactorization_Cython_Recommender",
         "MatrixFactorization_BPR_Cython": "MatrixFactorization_BPR_Cython_Recommender",
         "MatrixFactorization_FunkSVD_Cython": "MatrixFactorization_FunkSVD_Cython_Recommender",
         "MatrixFactorization_AsySVD_Cython": "MatrixFactorization_AsySVD_Cython_Recommender"}


def test_import_path_and_names():
    import MatrixFactorization.Cython.MatrixFactorization_Cython as M
    from ganmf_amd import MF_SGD
    from ganmf_amd.factor_model import FactorModelMixin
    from ganmf_amd.incremental_training import EarlyStoppingMixin
    for name, recommender_name in NAMES.items():
        cls = getattr(M, name)
        assert cls.__module__ == "MatrixFactorization.Cython.MatrixFactorization_Cython" and issubclass(cls, getattr(MF_SGD, name))
        assert cls.RECOMMENDER_NAME == recommender_name
        assert issubclass(cls, EarlyStoppingMixin) and issubclass(cls, FactorModelMixin)
    from MatrixFactorization.IALSRecommender import IALSRecommender      # the parent package still resolves its own modules
    assert IALSRecommender.RECOMMENDER_NAME == "IALSRecommender"


def test_signatures():
    from MatrixFactorization.Cython.MatrixFactorization_Cython import _MatrixFactorization_Cython, MatrixFactorization_BPR_Cython
    init = inspect.signature(_MatrixFactorization_Cython.__init__)
    assert [(n, p.default) for n, p in list(init.parameters.items())[2:]] == [("recompile_cython", False), ("algorithm_name", "MF_BPR"),
                                                                               ("device", 0), ("verbose", False)]
    fit = inspect.signature(_MatrixFactorization_Cython.fit)
    want = [("epochs", 300), ("batch_size", 1000), ("num_factors", 10), ("positive_threshold_BPR", None), ("learning_rate", 0.001),
            ("use_bias", True), ("sgd_mode", "sgd"), ("negative_interactions_quota", 0.0), ("init_mean", 0.0), ("init_std_dev", 0.1),
            ("user_reg", 0.0), ("item_reg", 0.0), ("bias_reg", 0.0), ("positive_reg", 0.0), ("negative_reg", 0.0), ("verbose", False),
            ("random_seed", None)]
    params = list(fit.parameters.items())
    assert [(n, p.default) for n, p in params[1:-1]] == want
    assert params[-1][0] == "earlystopping_kwargs" and params[-1][1].kind is inspect.Parameter.VAR_KEYWORD
    sub = list(inspect.signature(MatrixFactorization_BPR_Cython.fit).parameters.values())
    assert [p.kind for p in sub[1:]] == [inspect.Parameter.VAR_KEYWORD]      # fit(**key_args), as the reference's subclasses
    for method in ("recommend", "saveModel", "loadModel", "get_URM_train", "set_items_to_ignore", "_compute_item_score",
                   "_prepare_model_for_validation", "_update_best_model", "_run_epoch", "get_early_stopping_final_epochs_dict"):
        assert callable(getattr(_MatrixFactorization_Cython, method))
    for member in ("USER_factors", "ITEM_factors", "USER_bias", "ITEM_bias", "GLOBAL_bias", "USER_factors_best", "ITEM_factors_best"):
        assert isinstance(getattr(_MatrixFactorization_Cython, member), property)


def test_constructor_and_contract():
    from MatrixFactorization.Cython.MatrixFactorization_Cython import (MatrixFactorization_AsySVD_Cython, MatrixFactorization_BPR_Cython,
                                                                       MatrixFactorization_FunkSVD_Cython)
    urm = sps.random(12, 7, density=0.3, format="csr", dtype=np.float32, random_state=1)
    for cls, algorithm in ((MatrixFactorization_BPR_Cython, "MF_BPR"), (MatrixFactorization_FunkSVD_Cython, "FUNK_SVD"),
                           (MatrixFactorization_AsySVD_Cython, "ASY_SVD")):
        m = cls(urm, recompile_cython=True)
        assert (m.n_users, m.n_items, m.algorithm_name, m.normalize) == (12, 7, algorithm, False)
        assert m.mode == "user" and m.score_contract == "mf" and m.mask_cold_users is True      # as IALSRecommender
        with pytest.raises(RuntimeError):
            m.USER_factors
        with pytest.raises(TypeError):
            cls(urm, algorithm_name="MF_BPR")      # the subclasses fix it, as in the reference
    with pytest.raises(NotImplementedError, match="ASY_SVD is not implemented"):
        MatrixFactorization_AsySVD_Cython(urm).fit(epochs=1)


def test_the_entries_are_declared_and_bound():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    text = open(os.path.join(ROOT, "include", "ganmf_hip.h")).read()
    for name in ("init", "draw", "run", "epochs", "publish", "get_state", "set_state"):
        assert re.search(r"\nint ganmf_mf_sgd_%s\(ganmf_handle\* h" % name, text)
        assert "ganmf_mf_sgd_" + name in L.SYMBOLS
    assert text.index("int ganmf_mf_sgd_init(") > text.index("const char* ganmf_last_error(void);")      # appended: nothing moved
    for name, key in (("BPR", "MF_BPR"), ("FUNK", "FUNK_SVD")):
        assert int(re.search(r"GANMF_MF_SGD_%s = (\d+)" % name, text).group(1)) == L.MF_SGD_ALGORITHMS[key]
    for name in ("AUTO", "SEQUENTIAL", "LEVELLED"):
        assert int(re.search(r"GANMF_MF_SGD_%s = (\d+)" % name, text).group(1)) == getattr(L, "MF_SGD_" + name)
    assert int(re.search(r"#define GANMF_MF_SGD_MAX_FACTORS (\d+)", text).group(1)) == L.MF_SGD_MAX_FACTORS
    assert int(re.search(r"#define GANMF_MF_SGD_MAX_BATCH \(1 << (\d+)\)", text).group(1)) == L.MF_SGD_MAX_BATCH.bit_length() - 1
    assert int(re.search(r"#define GANMF_ABI_VERSION (\d+)", text).group(1)) == L.ABI_VERSION == 2
    for method in ("mf_sgd_init", "mf_sgd_draw", "mf_sgd_run", "mf_sgd_epochs", "mf_sgd_publish", "mf_sgd_state", "mf_sgd_set_state"):
        assert callable(getattr(Engine, method))
    # the generator and the sampler kernel are shared with SLIM-BPR, not copied
    csrc = os.path.join(ROOT, "ganmf_amd", "csrc")
    draw = open(os.path.join(csrc, "counter_draw.hpp")).read()
    assert draw.count("unsigned long long draw_mix(unsigned long long z) {") == 1 and draw.count("void draw_kernel(const DrawP p) {") == 1
    for header in ("slim_bpr.hpp", "mf_sgd.hpp"):
        text = open(os.path.join(csrc, header)).read()
        assert '#include "counter_draw.hpp"' in text
        assert "draw_mix(" not in text.split("#pragma once")[1] and "__global__" in text and "draw_kernel(const" not in text


def test_driver_import_sequence_with_reference_tree_behind(tmp_path):
    """this repository's root AHEAD of a stand-in reference tree: the class modules resolve here, the reference's epoch module (and
    any other module of its MatrixFactorization/Cython/ directory) still resolves there"""
    ref = tmp_path / "reference_tree" / "MatrixFactorization"
    (ref / "Cython").mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "Cython" / "__init__.py").write_text("")
    (ref / "Cython" / "MatrixFactorization_Cython.py").write_text("raise ImportError('the reference class module must be shadowed')\n")
    (ref / "Cython" / "MatrixFactorization_Cython_Epoch.py").write_text("MARK = 'reference epoch module'\n")
    (ref / "NMFRecommender.py").write_text("class NMFRecommender(object):\n    RECOMMENDER_NAME = 'NMFRecommender'\n")
    script = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        from MatrixFactorization.Cython.MatrixFactorization_Cython import MatrixFactorization_BPR_Cython, MatrixFactorization_FunkSVD_Cython
        from MatrixFactorization.Cython.MatrixFactorization_Cython import MatrixFactorization_AsySVD_Cython
        from MatrixFactorization.PureSVDRecommender import PureSVDRecommender
        from MatrixFactorization.NMFRecommender import NMFRecommender
        from MatrixFactorization.Cython.MatrixFactorization_Cython_Epoch import MARK
        import ganmf_amd.MF_SGD
        assert issubclass(MatrixFactorization_BPR_Cython, ganmf_amd.MF_SGD.MatrixFactorization_BPR_Cython)
        assert issubclass(MatrixFactorization_FunkSVD_Cython, ganmf_amd.MF_SGD.MatrixFactorization_FunkSVD_Cython)
        assert MatrixFactorization_BPR_Cython.RECOMMENDER_NAME == 'MatrixFactorization_BPR_Cython_Recommender'
        assert MatrixFactorization_BPR_Cython.__module__.split('.')[0] == 'MatrixFactorization'
        assert MARK == 'reference epoch module' and NMFRecommender.RECOMMENDER_NAME == 'NMFRecommender'
        print('OK')
    """) % (ROOT, str(tmp_path / "reference_tree"))
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
