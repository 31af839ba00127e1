"""The reference's import path for PureSVD: `MatrixFactorization.PureSVDRecommender.PureSVDRecommender` resolves to this repository's
class, as `MatrixFactorization.IALSRecommender.IALSRecommender` does for the ALS baseline."""
import importlib
import inspect

import numpy as np
import scipy.sparse as sps


def test_import_sequence_of_the_reference_drivers():
    from MatrixFactorization.PureSVDRecommender import PureSVDRecommender
    import ganmf_amd
    from ganmf_amd.PureSVD import PureSVDRecommender as Native
    from ganmf_amd.device_scoring import DeviceScoringMixin
    from ganmf_amd.factor_model import FactorModelMixin
    assert issubclass(PureSVDRecommender, Native) and issubclass(PureSVDRecommender, DeviceScoringMixin)
    assert issubclass(PureSVDRecommender, FactorModelMixin)
    assert ganmf_amd.PureSVDRecommender is Native and "PureSVDRecommender" in ganmf_amd.__all__
    assert PureSVDRecommender.RECOMMENDER_NAME == "PureSVDRecommender"
    assert PureSVDRecommender.__module__.split(".")[0] == "MatrixFactorization"
    # the package extends its search path like GANRec: another MatrixFactorization/ directory on sys.path stays reachable
    pkg = importlib.import_module("MatrixFactorization")
    assert hasattr(pkg, "__path__") and "extend_path" in inspect.getsource(pkg)
    assert "PureSVDRecommender" in pkg.__doc__


def test_constructor_and_fit_signature_are_the_reference_s():
    from MatrixFactorization.PureSVDRecommender import PureSVDRecommender
    sig = inspect.signature(PureSVDRecommender.fit)
    assert [(n, p.default) for n, p in sig.parameters.items() if n != "self"] == [("num_factors", 100)]
    model = PureSVDRecommender(sps.csr_matrix(np.eye(4, 6, dtype=np.float32)))
    assert (model.n_users, model.n_items) == (4, 6) and model.get_URM_train().shape == (4, 6)
    assert model.Sigma is None


def test_both_factor_models_share_the_engine_plumbing_and_persistence():
    from ganmf_amd.IALS import IALSRecommender
    from ganmf_amd.PureSVD import PureSVDRecommender
    for name in ["_make_engine", "_build", "_require_engine", "saveModel", "loadModel", "_zip_path", "recommend", "activity_study"]:
        assert getattr(IALSRecommender, name) is getattr(PureSVDRecommender, name), name
    assert IALSRecommender.USER_factors is PureSVDRecommender.USER_factors
