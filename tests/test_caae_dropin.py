"""CAAE as a drop-in: with a stand-in reference tree BEHIND the repository (as in test_dropin_imports.py) `GANRec.CAAE.CAAE` is this
repository's class under the reference's import path; its name and signatures; the binding of the ganmf_caae_* entries.  No GPU."""
import inspect
import os
import re
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_caae_resolves_here_with_a_reference_tree_behind(tmp_path):
    ref = tmp_path / "reference_tree" / "GANRec"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "CAAE.py").write_text("raise ImportError('the reference CAAE (TensorFlow) must be shadowed')\n")
    (ref / "Other.py").write_text("VALUE = 'reference'\n")
    script = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        from GANRec.CAAE import CAAE
        import ganmf_amd.CAAE
        import ganmf_amd._lib as L
        assert L._lib is None                                     # importing the class does not load the library
        assert CAAE.__module__ == 'GANRec.CAAE' and CAAE.__module__.split('.')[0] == 'GANRec'      # the driver's isGAN test
        assert issubclass(CAAE, ganmf_amd.CAAE.CAAE) and ganmf_amd.CAAE.CAAE.__module__ == 'ganmf_amd.CAAE'
        assert CAAE.RECOMMENDER_NAME == 'CAAE'
        import ganmf_amd
        assert 'CAAE' in ganmf_amd.__all__
        from GANRec.Other import VALUE                            # extend_path still reaches the reference's other modules
        assert VALUE == 'reference'
        print('OK')
    """) % (ROOT, str(tmp_path / "reference_tree"))
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr


def test_signatures_and_documented_quirks():
    from GANRec.CAAE import CAAE
    init = inspect.signature(CAAE.__init__)
    assert [(n, p.default) for n, p in list(init.parameters.items())[2:6]] == [("verbose", False), ("mode", "user"), ("seed", 1234),
                                                                                ("is_experiment", False)]
    assert list(inspect.signature(CAAE.fit).parameters)[1:8] == ["epochs", "d_steps", "g_steps", "gpr_steps", "g_layers", "g_units",
                                                                  "gpr_layers"]
    assert list(inspect.signature(CAAE.saveModel).parameters) == ["self", "folder_path", "file_name"]
    for method in ("stop_fit", "save_current_model", "load_model", "_compute_item_score", "recommend", "load_bundle"):
        assert callable(getattr(CAAE, method))
    doc = CAAE.__mro__[1].__doc__
    for quirk in ("`mode` is stored", "gpr_layers and gpr_units", "stored profile values", "int(n_free * S)", "epoch - 1",
                  "scores the users it is asked for", "log1p", "sampler=\"numpy\"", "RandomState(seed)", "stored zeros"):
        assert quirk in doc, quirk


def test_the_entries_are_declared_and_bound():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    text = open(os.path.join(ROOT, "include", "ganmf_hip.h")).read()
    for name in ("init", "cdf", "draw_perm", "draw_negatives", "draw_batch", "get_draws", "d_step", "g_step", "epoch"):
        assert re.search(r"\nint ganmf_caae_%s\(ganmf_handle\* h" % name, text)
        assert "ganmf_caae_" + name in L.SYMBOLS
    assert int(re.search(r"GANMF_MODEL_CAAE = (\d+)", text).group(1)) == L.MODEL_CAAE == 5
    assert int(re.search(r"#define GANMF_T_CAAE_ITEM_BIAS (\d+)", text).group(1)) == L.T_CAAE_ITEM_BIAS
    assert int(re.search(r"#define GANMF_T_CAAE_G0 (\d+)", text).group(1)) == L.T_CAAE_G0
    assert int(re.search(r"#define GANMF_T_CAAE_GPR0 (\d+)", text).group(1)) == L.T_CAAE_GPR0
    assert int(re.search(r"#define GANMF_CAAE_MAX_FACTORS (\d+)", text).group(1)) == L.CAAE_MAX_FACTORS
    assert int(re.search(r"#define GANMF_CAAE_MAX_D_BSIZE (\d+)", text).group(1)) == L.CAAE_MAX_D_BSIZE
    for name, value in L.CAAE_DRAWS.items():
        assert int(re.search(r"GANMF_CAAE_DRAW_%s = (\d+)" % name.upper(), text).group(1)) == value
    assert int(re.search(r"#define GANMF_ABI_VERSION (\d+)", text).group(1)) == L.ABI_VERSION == 2
    for method in ("caae_init", "caae_cdf", "caae_draw_perm", "caae_draw_negatives", "caae_draw_batch", "caae_draws", "caae_d_step",
                   "caae_g_step", "caae_epoch"):
        assert callable(getattr(Engine, method))


def test_tuning_stays_out_of_scope():
    from ganmf_amd import tune
    with pytest.raises(Exception):
        tune.search_space("CAAE")
