"""SLIM_BPR_Cython as a drop-in: the reference's import path, name and signatures (SLIM_BPR/Cython/SLIM_BPR_Cython.py:50-85), the
refusals, and the binding of the ganmf_slim_bpr_* entries."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_import_path_and_name():
    from SLIM_BPR.Cython.SLIM_BPR_Cython import SLIM_BPR_Cython
    from ganmf_amd import SLIM_BPR
    from ganmf_amd.incremental_training import EarlyStoppingMixin
    from ganmf_amd.similarity_model import SimilarityModelMixin
    assert SLIM_BPR_Cython.__module__ == "SLIM_BPR.Cython.SLIM_BPR_Cython" and issubclass(SLIM_BPR_Cython, SLIM_BPR.SLIM_BPR_Cython)
    assert SLIM_BPR_Cython.RECOMMENDER_NAME == "SLIM_BPR_Recommender"
    assert issubclass(SLIM_BPR_Cython, SimilarityModelMixin) and issubclass(SLIM_BPR_Cython, EarlyStoppingMixin)
    from MatrixFactorization.IALSRecommender import IALSRecommender
    assert issubclass(IALSRecommender, EarlyStoppingMixin)      # one early-stopping loop for both


def test_signatures():
    from SLIM_BPR.Cython.SLIM_BPR_Cython import SLIM_BPR_Cython
    init = inspect.signature(SLIM_BPR_Cython.__init__)
    assert list(init.parameters)[:4] == ["self", "URM_train", "free_mem_threshold", "recompile_cython"]
    assert init.parameters["free_mem_threshold"].default == 0.5 and init.parameters["recompile_cython"].default is False
    assert all(p.default is not inspect.Parameter.empty for p in list(init.parameters.values())[2:])
    fit = inspect.signature(SLIM_BPR_Cython.fit)
    want = [("epochs", 300), ("positive_threshold_BPR", None), ("train_with_sparse_weights", None), ("symmetric", True), ("verbose", False),
            ("random_seed", None), ("batch_size", 1000), ("lambda_i", 0.0), ("lambda_j", 0.0), ("learning_rate", 1e-4), ("topK", 200),
            ("sgd_mode", "adagrad"), ("gamma", 0.995), ("beta_1", 0.9), ("beta_2", 0.999)]
    params = list(fit.parameters.items())
    assert [(n, p.default) for n, p in params[1:-1]] == want
    assert params[-1][0] == "earlystopping_kwargs" and params[-1][1].kind is inspect.Parameter.VAR_KEYWORD
    es = inspect.signature(SLIM_BPR_Cython._train_with_early_stopping)
    assert list(es.parameters)[1:] == ["epochs_max", "epochs_min", "validation_every_n", "stop_on_validation", "validation_metric",
                                       "lower_validations_allowed", "evaluator_object"]
    for method in ("recommend", "saveModel", "loadModel", "get_URM_train", "set_items_to_ignore", "_compute_item_score",
                   "_prepare_model_for_validation", "_update_best_model", "_run_epoch", "get_S_incremental_and_set_W",
                   "get_early_stopping_final_epochs_dict"):
        assert callable(getattr(SLIM_BPR_Cython, method))
    assert isinstance(SLIM_BPR_Cython.W_sparse, property) and isinstance(SLIM_BPR_Cython.S_incremental, property)


def test_constructor_and_refusals():
    from SLIM_BPR.Cython.SLIM_BPR_Cython import SLIM_BPR_Cython
    urm = sps.random(12, 7, density=0.3, format="csr", dtype=np.float32, random_state=1)
    m = SLIM_BPR_Cython(urm, recompile_cython=True)
    assert (m.n_users, m.n_items) == (12, 7) and m.get_URM_train().shape == (12, 7)
    assert m.mode == "user" and m.score_contract == "mf" and m.mask_cold_users is False and m.honours_items_to_compute is True
    with pytest.raises(ValueError, match="train_with_sparse_weights=True"):
        m.fit(epochs=1, train_with_sparse_weights=True)
    with pytest.raises(ValueError, match="TopK not valid"):
        m.fit(epochs=1, topK=-3)
    with pytest.raises(ValueError, match="SGD_mode not valid"):
        m.fit(epochs=1, sgd_mode="nesterov")
    with pytest.raises(AssertionError, match="free_mem_threshold"):
        SLIM_BPR_Cython(urm, free_mem_threshold=-0.1)
    with pytest.raises(NotImplementedError):
        m.recommend_candidates(np.arange(2), None)
    with pytest.raises(RuntimeError):
        m.W_sparse
    with pytest.raises(RuntimeError):
        m.S_incremental


def test_the_entries_are_declared_and_bound():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    text = open(os.path.join(ROOT, "include", "ganmf_hip.h")).read()
    for name in ("init", "draw", "run", "epochs", "finish", "get_state"):
        assert re.search(r"\nint ganmf_slim_bpr_%s\(ganmf_handle\* h" % name, text)
        assert "ganmf_slim_bpr_" + name in L.SYMBOLS
    for name, value in L.SLIM_SGD_MODES.items():
        assert int(re.search(r"GANMF_SLIM_%s = (\d+)" % name.upper(), text).group(1)) == value
    for name in ("AUTO", "SEQUENTIAL", "LEVELLED"):
        assert int(re.search(r"GANMF_SLIM_%s = (\d+)" % name, text).group(1)) == getattr(L, "SLIM_" + name)
    assert int(re.search(r"#define GANMF_ABI_VERSION (\d+)", text).group(1)) == L.ABI_VERSION == 2
    for method in ("slim_bpr_init", "slim_bpr_draw", "slim_bpr_run", "slim_bpr_epochs", "slim_bpr_finish", "slim_bpr_state"):
        assert callable(getattr(Engine, method))
    # the restated constants are the kernels'
    from tests import helpers_slim_bpr as H
    csrc = os.path.join(ROOT, "ganmf_amd", "csrc")
    assert int(re.search(r"constexpr int DRAW_ATTEMPTS = (\d+);", open(os.path.join(csrc, "counter_draw.hpp")).read()).group(1)) == H.ATTEMPTS
    assert int(re.search(r"constexpr int SLIM_THREADS = (\d+);", open(os.path.join(csrc, "slim_bpr.hpp")).read()).group(1)) == H.THREADS
