"""The reference's import path for NMF: `MatrixFactorization.NMFRecommender.NMFRecommender` resolves to this repository's class, as
`MatrixFactorization.PureSVDRecommender.PureSVDRecommender` and `MatrixFactorization.IALSRecommender.IALSRecommender` do."""
import importlib
import inspect

import numpy as np
import scipy.sparse as sps


def test_import_sequence_of_the_reference_drivers():
    from MatrixFactorization.NMFRecommender import NMFRecommender
    import ganmf_amd
    from ganmf_amd.NMF import NMFRecommender as Native
    from ganmf_amd.device_scoring import DeviceScoringMixin
    from ganmf_amd.factor_model import FactorModelMixin
    assert issubclass(NMFRecommender, Native) and issubclass(NMFRecommender, DeviceScoringMixin)
    assert issubclass(NMFRecommender, FactorModelMixin)
    assert ganmf_amd.NMFRecommender is Native and "NMFRecommender" in ganmf_amd.__all__
    assert NMFRecommender.RECOMMENDER_NAME == "NMFRecommender"
    assert NMFRecommender.__module__.split(".")[0] == "MatrixFactorization"
    pkg = importlib.import_module("MatrixFactorization")
    assert hasattr(pkg, "__path__") and "extend_path" in inspect.getsource(pkg)
    for name in ["NMFRecommender", "PureSVDRecommender", "IALSRecommender"]:      # the package's docstring keeps naming all three
        assert name in pkg.__doc__


def test_constructor_fit_signature_and_class_attributes_are_the_reference_s():
    from MatrixFactorization.NMFRecommender import NMFRecommender
    sig = inspect.signature(NMFRecommender.fit)
    assert [(n, p.default) for n, p in sig.parameters.items() if n != "self"] == [
        ("num_factors", 100), ("l1_ratio", 0.5), ("solver", "multiplicative_update"), ("init_type", "random"),
        ("beta_loss", "frobenius"), ("verbose", False)]
    assert NMFRecommender.SOLVER_VALUES == {"coordinate_descent": "cd", "multiplicative_update": "mu"}
    assert NMFRecommender.INIT_VALUES == ["random", "nndsvda"]
    assert NMFRecommender.BETA_LOSS_VALUES == ["frobenius", "kullback-leibler"]
    assert list(inspect.signature(NMFRecommender.__init__).parameters)[:2] == ["self", "URM_train"]
    model = NMFRecommender(sps.csr_matrix(np.eye(4, 6, dtype=np.float32)))
    assert (model.n_users, model.n_items) == (4, 6) and model.get_URM_train().shape == (4, 6)
    assert model.n_iter_ is None and model.reconstruction_err_ is None and model.transform_n_iter_ is None
    assert model.score_contract == "mf"


def test_limits_are_stated():
    from ganmf_amd import _lib as L
    from ganmf_amd.NMF import NMFRecommender
    assert NMFRecommender.MAX_FACTORS == 270 == L.NMF_MAX_FACTORS == L.SVD_MAX_RANDOM - NMFRecommender.OVERSAMPLES
    assert "270" not in NMFRecommender.MAX_FACTORS_REASON and "nndsvda" in NMFRecommender.MAX_FACTORS_REASON
    assert (NMFRecommender.MAX_ITER, NMFRecommender.TOL) == (500, 1e-4)
    for name in ("ganmf_nmf_mu", "ganmf_nmf_cd", "ganmf_nmf_error"):
        assert name in L.SYMBOLS


def test_the_factor_models_share_the_engine_plumbing_and_persistence():
    from ganmf_amd.NMF import NMFRecommender
    from ganmf_amd.PureSVD import PureSVDRecommender
    for name in ["_make_engine", "_build", "_require_engine", "saveModel", "loadModel", "_zip_path", "recommend", "activity_study"]:
        assert getattr(NMFRecommender, name) is getattr(PureSVDRecommender, name), name
    assert NMFRecommender.USER_factors is PureSVDRecommender.USER_factors
