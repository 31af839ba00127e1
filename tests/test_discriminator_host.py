"""Host side of discriminator inference (no GPU): the study's arithmetic, the restatements of tests/helpers_discriminator.py against
the oracle's own batch loss, the float32 restatement's deviation beside each floor at the GPU test's shapes, and the class methods'
behaviour before fit()."""
import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.studies import discriminator_summary
from oracle.ganmf_oracle import GANMFOracle
from tests import helpers_discriminator as H


def test_summary_energies_and_hinge():
    real, gen = np.array([0.5, 1.5, 1.0]), np.array([2.0, 4.0])
    s = discriminator_summary(real, gen, m=2.5)
    assert s["mean_real"] == 1.0 and s["mean_generated"] == 3.0
    assert s["hinge"] == 2.5 * 1.0 - 3.0 and s["hinge_active"] is False
    assert discriminator_summary(real, gen, m=4.0)["hinge_active"] is True
    assert s["energy_real"].dtype == np.float64 and s["energy_real"].shape == (3,) and s["energy_generated"].shape == (2,)
    none = discriminator_summary(real, gen, m=None)
    assert none["hinge"] is None and none["hinge_active"] is None and none["mean_real"] == 1.0


def test_summary_logits():
    real, gen = np.array([2.0, -1.0, 0.0, 3.0]), np.array([-2.0, 1.0])
    s = discriminator_summary(real, gen, logits=True)
    np.testing.assert_allclose(s["p_real"], 1.0 / (1.0 + np.exp(-real)), rtol=1e-15)
    np.testing.assert_allclose(s["p_generated"], 1.0 / (1.0 + np.exp(-gen)), rtol=1e-15)
    assert s["mean_p_real"] == pytest.approx(s["p_real"].mean()) and s["mean_p_generated"] == pytest.approx(s["p_generated"].mean())
    assert s["accuracy"] == 0.5 * (2 / 4 + 1 / 2)      # a logit of exactly 0 is on neither side


def test_mean_of_row_energies_is_the_batch_loss():
    """mean over a batch of oracle64's per-row energies == the loss GANMFOracle.autoencoder returns for that batch"""
    U, N, k, e = H.DOMAIN, 70, H.K_FACTORS, 8
    w, urm = H.ganmf_weights(U, N, k, e, 3), H.make_urm(U, N, 4)
    ids = H.make_ids(U, 65, 5)
    o = GANMFOracle(U, N, k, e, dtype=np.float64)
    o.set_params(**w)
    for generated in (False, True):
        inp = o.generator(ids) if generated else urm[ids].toarray().astype(np.float64)
        E, _, loss = o.autoencoder(inp)
        codes, energy = H.oracle64(w, urm, ids, generated)
        np.testing.assert_array_equal(codes, E)
        assert abs(energy.mean() - loss) <= 4 * np.finfo(np.float64).eps * loss


def test_restatement_deviation_beside_the_floors():
    """The yardstick at the GPU test's shapes: the float32 restatement's own deviation from float64, printed beside each floor.
    (Checked here: the deviation is a float32 rounding effect -- well under 1e-4 -- and the energies keep clear of cancellation.)"""
    U, k = H.DOMAIN, H.K_FACTORS
    print()
    for N in (70, 257):
        for e in (8, 72):
            w, urm = H.ganmf_weights(U, N, k, e, 10 + e), H.make_urm(U, N, N)
            ids = H.make_ids(U, 257, 6)
            for generated in (False, True):
                (c64, v64), (c32, v32) = H.oracle64(w, urm, ids, generated), H.restatement32(w, urm, ids, generated)
                dc, dv = H.deviations(c32, c64, False), H.deviations(v32, v64, True)
                print("GANMF N=%d e=%d generated=%d: codes restatement %.2e floor %.2e | energies restatement %.2e floor %.2e "
                      "(energies %.2e .. %.2e)" % (N, e, generated, dc, H.floor_of("codes", N, c64), dv, H.floor_of("energy", N, v64),
                                                  v64.min(), v64.max()))
                assert dc < 1e-4 and dv < 1e-4 and v64.min() > 1e-4
            for act in ("linear", "tanh"):
                for layers in (1, 2):
                    wd = H.disganmf_weights(U, N, k, layers, e, 20 + e)
                    for generated in (False, True):
                        (f64, l64), (f32, l32) = H.oracle64(wd, urm, ids, generated, act), H.restatement32(wd, urm, ids, generated, act)
                        df, dl = H.deviations(f32, f64, False), H.deviations(l32, l64, False)
                        print("DisGANMF N=%d nodes=%d %s x%d generated=%d: features restatement %.2e floor %.2e | logits restatement "
                              "%.2e floor %.2e" % (N, e, act, layers, generated, df, H.floor_of("features", N, f64), dl,
                                                   H.floor_of("logit", N, l64)))
                        assert df < 1e-4 and dl < 1e-4


def test_ids_and_matrix_have_the_edge_rows():
    urm = H.make_urm(H.DOMAIN, 70, 1)
    assert urm[0].nnz == 0 and urm[1].nnz == 70
    assert set(np.unique(H.make_urm(H.DOMAIN, 70, 1, binary=False).data)) - {1.0} != set()
    for n in (1, 63, 64, 65, 129, 257):
        ids = H.make_ids(H.DOMAIN, n, 2)
        assert ids.shape == (n,) and ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < H.DOMAIN
        if n > 1:
            assert ids[-1] == ids[0] and len(np.unique(ids)) == n - 1
        if n > 2:
            assert 0 in ids and 1 in ids


def test_methods_need_device_state():
    """before fit() / loadModel() the new methods raise the classes' existing error"""
    from ganmf_amd.DisGANMF import DisGANMF
    from ganmf_amd.GANMF import GANMF
    urm = sps.csr_matrix(np.eye(4, 5, dtype=np.float32))
    g = GANMF(urm, is_experiment=True)
    for call in (g.autoencoder_codes, g.discriminator_energy, g.discriminator_study,
                 lambda: g.autoencoder_codes([0], generated=True)):
        with pytest.raises(RuntimeError, match="no device state"):
            call()
    d = DisGANMF(urm, is_experiment=True)
    for call in (d.discriminator_logits, d.discriminator_study, lambda: d.discriminator_logits([1], True, True)):
        with pytest.raises(RuntimeError, match="no device state"):
            call()
    with pytest.raises(AttributeError):
        d.autoencoder_codes()


def test_entry_points_are_declared_and_bound():
    import os
    import re
    from ganmf_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ganmf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ganmf_discriminate", "ganmf_set_discriminate_block"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in L.SYMBOLS
    assert "#define GANMF_ABI_VERSION 2" in header
