"""The reference's import path for the ALS baseline: `MatrixFactorization.IALSRecommender.IALSRecommender` (RecSysExp.py,
RunBestParameters.py) resolves to this repository's class, as `GANRec.GANMF.GANMF` does for the GAN models."""
import importlib
import inspect

import numpy as np
import scipy.sparse as sps


def test_import_sequence_of_the_reference_drivers():
    from MatrixFactorization.IALSRecommender import IALSRecommender
    import ganmf_amd
    from ganmf_amd.IALS import IALSRecommender as Native
    from ganmf_amd.device_scoring import DeviceScoringMixin
    assert issubclass(IALSRecommender, Native) and issubclass(IALSRecommender, DeviceScoringMixin)
    assert ganmf_amd.IALSRecommender is Native
    assert IALSRecommender.RECOMMENDER_NAME == "IALSRecommender"
    assert IALSRecommender.__module__.split(".")[0] == "MatrixFactorization"
    # the package extends its search path like GANRec: another MatrixFactorization/ directory on sys.path stays reachable
    pkg = importlib.import_module("MatrixFactorization")
    assert hasattr(pkg, "__path__") and "extend_path" in inspect.getsource(pkg)


def test_fit_signature_is_the_reference_s():
    from MatrixFactorization.IALSRecommender import IALSRecommender
    sig = inspect.signature(IALSRecommender.fit)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self" and p.kind != p.VAR_KEYWORD]
    assert got == [("epochs", 300), ("num_factors", 20), ("confidence_scaling", "linear"), ("alpha", 1.0), ("epsilon", 1.0),
                   ("reg", 1e-3), ("init_mean", 0.0), ("init_std", 0.1)]
    assert any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values())
    ts = inspect.signature(IALSRecommender._train_with_early_stopping)
    assert [n for n in ts.parameters][1:] == ["epochs_max", "epochs_min", "validation_every_n", "stop_on_validation",
                                              "validation_metric", "lower_validations_allowed", "evaluator_object"]
    model = IALSRecommender(sps.csr_matrix(np.eye(4, 6, dtype=np.float32)))
    assert (model.n_users, model.n_items) == (4, 6) and model.get_URM_train().shape == (4, 6)
    assert model.AVAILABLE_CONFIDENCE_SCALING == ["linear", "log"]


def test_ganmf_keeps_its_surface_through_the_mixin():
    """the device-scoring methods moved out of GANMF.py: GANMF and DisGANMF still have every one of them"""
    from ganmf_amd.DisGANMF import DisGANMF
    from ganmf_amd.GANMF import GANMF
    from ganmf_amd.IALS import IALSRecommender
    names = ["_compute_item_score", "recommend", "recommend_topk", "evaluate_on_device", "evaluate_full_on_device",
             "evaluate_candidates_on_device", "evaluate_groups_on_device", "evaluate_diversity_on_device", "recommend_candidates",
             "prediction_similarity", "activity_study", "_ignored_items", "_item_filter", "honours_items_to_compute"]
    for cls in (GANMF, DisGANMF, IALSRecommender):
        for n in names:
            assert hasattr(cls, n), (cls, n)
    assert GANMF.recommend is IALSRecommender.recommend
