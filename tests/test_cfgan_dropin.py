"""CFGAN as a drop-in: the reference's import path, name and signatures (GANRec/CFGAN.py:25,112-115), the refusals, and the binding
of the ganmf_cfgan_* entries.  No GPU."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_import_does_not_load_the_library():
    code = ("import sys; sys.path.insert(0, %r); import GANRec.CFGAN as m; import ganmf_amd._lib as L; "
            "assert L._lib is None; assert m.CFGAN.__module__ == 'GANRec.CFGAN'; print('ok')" % ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr


def test_import_path_and_name():
    from GANRec.CFGAN import CFGAN
    from ganmf_amd.CFGAN import CFGAN as impl
    assert CFGAN.__module__.split(".")[0] == "GANRec" and CFGAN.RECOMMENDER_NAME == "CFGAN"
    assert issubclass(CFGAN, impl) and impl.__module__ == "ganmf_amd.CFGAN"


def test_signatures_are_the_references():
    from GANRec.CFGAN import CFGAN
    init = inspect.signature(CFGAN.__init__)
    assert [(n, p.default) for n, p in list(init.parameters.items())[2:6]] == [("mode", "user"), ("seed", 1234), ("verbose", False),
                                                                                ("is_experiment", False)]
    want = [("d_nodes", 32), ("g_nodes", 32), ("d_layers", 1), ("g_layers", 1), ("scheme", "ZR"), ("d_hidden_act", "linear"),
            ("g_hidden_act", "linear"), ("epochs", 300), ("d_lr", 1e-5), ("g_lr", 1e-5), ("d_reg", 0), ("g_reg", 0), ("d_steps", 1),
            ("g_steps", 1), ("d_batch_size", 32), ("g_batch_size", 32), ("zr_ratio", 0.), ("zp_ratio", 0.), ("zr_coefficient", 0.),
            ("allow_worse", 5), ("freq", 5), ("after", 0), ("metrics", ["MAP"]), ("validation_evaluator", None), ("sample_every", None),
            ("validation_set", None)]
    fit = inspect.signature(CFGAN.fit)
    assert [(n, p.default) for n, p in list(fit.parameters.items())[1:]] == want
    assert list(inspect.signature(CFGAN.saveModel).parameters) == ["self", "folder_path", "file_name"]
    for method in ("stop_fit", "save_current_model", "load_model", "_compute_item_score", "recommend", "load_bundle", "upload_masks"):
        assert callable(getattr(CFGAN, method))
    for quirk in ("zp_ratio", "np.float32(zr_ratio)", "epoch - 1", "LeakyReLU", "mask_sampler"):
        assert quirk in CFGAN.__mro__[1].__doc__


def test_constructor_and_refusals():
    from GANRec.CFGAN import CFGAN
    urm = sps.random(12, 7, density=0.3, format="csr", dtype=np.float32, random_state=1)
    u, i = CFGAN(urm, is_experiment=True), CFGAN(urm, mode="item", is_experiment=True)
    assert (u.num_users, u.num_items) == (12, 7) and (i.num_users, i.num_items) == (7, 12)
    assert i.URM_train.shape == (7, 12) and (i.n_users, i.n_items) == (12, 7)
    with pytest.raises(ValueError):
        CFGAN(urm, mode="both", is_experiment=True)
    with pytest.raises(ValueError, match="mask_sampler"):
        CFGAN(urm, mask_sampler="tf", is_experiment=True)
    with pytest.raises(ValueError, match="world_size"):
        CFGAN(urm, world_size=2, is_experiment=True)
    with pytest.raises(ValueError, match="mfma"):
        CFGAN(urm, mfma="bf16", is_experiment=True)
    with pytest.raises(ValueError, match="LeakyReLU"):
        u.fit(epochs=1, d_hidden_act="LeakyReLU")
    with pytest.raises(ValueError, match="scheme"):
        u.fit(epochs=1, scheme="ZZ")
    with pytest.raises(ValueError, match="d_layers >= 1"):
        u.fit(epochs=1, g_layers=0)
    with pytest.raises(RuntimeError):
        u._compute_item_score(np.arange(2))


def test_the_entries_are_declared_and_bound():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    text = open(os.path.join(ROOT, "include", "ganmf_hip.h")).read()
    for name in ("init", "draw_masks", "set_masks", "get_masks", "step", "epoch"):
        assert re.search(r"\nint ganmf_cfgan_%s\(ganmf_handle\* h" % name, text)
        assert "ganmf_cfgan_" + name in L.SYMBOLS
    assert int(re.search(r"GANMF_MODEL_CFGAN = (\d+)", text).group(1)) == L.MODEL_CFGAN == 4
    assert int(re.search(r"#define GANMF_T_CFGAN_G0 (\d+)", text).group(1)) == L.T_CFGAN_G0 == 200
    for name, value in L.CFGAN_SCHEMES.items():
        assert int(re.search(r"GANMF_CFGAN_%s = (\d+)" % name, text).group(1)) == value
    assert int(re.search(r"#define GANMF_ABI_VERSION (\d+)", text).group(1)) == L.ABI_VERSION == 2
    for method in ("cfgan_init", "cfgan_epoch", "cfgan_step", "cfgan_draw_masks", "cfgan_set_masks", "cfgan_masks"):
        assert callable(getattr(Engine, method))


def test_tuning_stays_out_of_scope():
    from ganmf_amd import tune
    with pytest.raises(Exception):
        tune.search_space("CFGAN")
