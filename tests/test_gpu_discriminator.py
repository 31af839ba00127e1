"""Discriminator inference on the device (ganmf_discriminate; GANMF.py:62-70,304-307, DisGANMF.py:57-65): codes and per-row EBGAN
energies of GANMF, last hidden features and logits of DisGANMF, for stored rows (CSR, never densified for GANMF) and generated rows.

Bound (the project's rule for fp32-accurate paths, tests/test_gpu_similarity.py): a deviation from the float64 oracle is allowed up to
max(4 x the deviation of the float32 restatement on the same inputs, floor), with the floors
    codes                  sqrt(N) 2^-23 max|E|
    energies               sqrt(N) 2^-23, relative, per row
    DisGANMF features      sqrt(N + 2) 2^-23 max|features|     (N + 2 input terms: profile, bias, float(uid))
    logits                 sqrt(N + 2) 2^-23 max|logit|
(tests/helpers_discriminator.py).  Every case prints `ratio = deviation / allowed`.
Shapes: a 300-row domain; N in {70, 257} (pad columns, a column-tile tail, the ones column); emb_dim / d_nodes in {8, 72} (one K-tile,
a K tail past one); k = 8; n in {1, 63, 64, 65, 129, 257} (row-tile tails, more than one row tile); ids a shuffled subset with one id
repeated; an empty row, a row with all N entries stored, one case with non-binary values."""
import ctypes as C
import functools
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_discriminator as H

pytestmark = pytest.mark.gpu

U_DOM, K = H.DOMAIN, H.K_FACTORS
N_LIST = (1, 63, 64, 65, 129, 257)
GANMF_IDS = {"We": 0, "be": 1, "Wd": 2, "bd": 3, "U": 100, "V": 101}
HP = dict(d_lr=1e-3, g_lr=1e-3, d_reg=0.0, g_reg=0.0, m=2.0, recon_coefficient=0.05)
SLOTS = (0, 1, 2)      # parameter, Adam m, Adam v


def _ganmf_engine(w, urm, B=64, mfma=None, hp=HP):
    from ganmf_amd.engine import Engine
    (U, k), (N, e) = w["U"].shape, w["We"].shape
    eng = Engine(U, N, k, e, B, mfma=mfma, **hp)
    eng.set_urm(urm)
    for name, tid in GANMF_IDS.items():
        eng.set_tensor(tid, w[name])
    return eng


def _dis_tids(layers):
    return list(range(2 * layers + 2)) + [100, 101]


def _dis_engine(w, urm, act, B=64, mfma=None):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    (U, k), N, nodes = w["U"].shape, w["V"].shape[0], w["W0"].shape[1]
    layers = (len(w) - 4) // 2
    hp = {n: v for n, v in HP.items() if n != "m"}
    eng = Engine(U, N, k, nodes, B, model=L.MODEL_DISGANMF, d_layers=layers, d_act=act, mfma=mfma, **hp)
    eng.set_urm(urm)
    for l in range(layers):
        eng.set_tensor(2 * l, w["W%d" % l])
        eng.set_tensor(2 * l + 1, w["b%d" % l])
    eng.set_tensor(2 * layers, w["Wo"])
    eng.set_tensor(2 * layers + 1, w["bo"])
    eng.set_tensor(100, w["U"])
    eng.set_tensor(101, w["V"])
    return eng


@functools.lru_cache(maxsize=None)
def _ganmf_case(N, e, binary=True):
    return H.ganmf_weights(U_DOM, N, K, e, 10 + e), H.make_urm(U_DOM, N, N, binary=binary)


@functools.lru_cache(maxsize=None)
def _refs(N, e, binary, n, generated):
    """(ids, oracle64, restatement32) of one GANMF case: computed once, shared by the tests that need it"""
    w, urm = _ganmf_case(N, e, binary)
    ids = H.make_ids(U_DOM, n, n)
    return ids, H.oracle64(w, urm, ids, generated), H.restatement32(w, urm, ids, generated)


def _check(label, N, got, ref64, ref32, kinds=("codes", "energy")):
    """prints every ratio = deviation / allowed of (features, value) and returns the largest"""
    worst = 0.0
    for kind, g, r64, r32 in zip(kinds, got, ref64, ref32):
        if g is None:
            continue
        assert g.shape == r64.shape, (label, kind, g.shape, r64.shape)
        r, dev, lim = H.ratio(kind, N, g, r64, r32)
        print("%s %s: deviation %.3e, allowed %.3e, ratio %.3f" % (label, kind, dev, lim, r))
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("generated", [False, True])
@pytest.mark.parametrize("N,e,binary", [(70, 8, True), (70, 72, False), (257, 8, True), (257, 72, True)])
def test_ganmf_codes_and_energies(N, e, binary, generated):
    w, urm = _ganmf_case(N, e, binary)
    eng = _ganmf_engine(w, urm)
    worst = 0.0
    print()
    for n in N_LIST:
        ids, r64, r32 = _refs(N, e, binary, n, generated)
        feat, val = eng.discriminate(ids, generated=generated)
        assert feat.dtype == np.float32 and val.dtype == np.float64 and feat.shape == (n, e) and val.shape == (n,)
        worst = max(worst, _check("GANMF N=%d e=%d generated=%d n=%d" % (N, e, generated, n), N, (feat, val), r64, r32))
        # either output alone is the same bytes
        np.testing.assert_array_equal(eng.discriminate(ids, generated=generated, value=False)[0], feat)
        np.testing.assert_array_equal(eng.discriminate(ids, generated=generated, features=False)[1], val)
        if not generated and 0 in ids:      # the empty row encodes to exactly the bias
            np.testing.assert_array_equal(feat[list(ids).index(0)], w["be"])
        if n > 1:                           # the repeated id repeats its row
            np.testing.assert_array_equal(feat[-1], feat[0])
            assert val[-1] == val[0]
    eng.close()
    assert worst <= 1.0, worst


@pytest.mark.parametrize("generated", [False, True])
@pytest.mark.parametrize("N,nodes", [(70, 8), (257, 72)])
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("act", ["linear", "tanh"])
def test_disganmf_features_and_logits(act, layers, N, nodes, generated):
    w, urm = H.disganmf_weights(U_DOM, N, K, layers, nodes, 20 + nodes), H.make_urm(U_DOM, N, N)
    eng = _dis_engine(w, urm, act)
    worst = 0.0
    print()
    for n in (1, 65, 257):
        ids = H.make_ids(U_DOM, n, n)
        r64, r32 = H.oracle64(w, urm, ids, generated, act), H.restatement32(w, urm, ids, generated, act)
        feat, logit = eng.discriminate(ids, generated=generated)
        assert feat.shape == (n, nodes) and logit.shape == (n,) and logit.dtype == np.float64
        worst = max(worst, _check("DisGANMF N=%d nodes=%d %s x%d generated=%d n=%d" % (N, nodes, act, layers, generated, n), N,
                                  (feat, logit), r64, r32, kinds=("features", "logit")))
        np.testing.assert_array_equal(eng.discriminate(ids, generated=generated, features=False)[1], logit)
    eng.close()
    assert worst <= 1.0, worst


@pytest.mark.parametrize("generated", [False, True])
def test_exact_on_representable_inputs(generated):
    """small-integer weights and binary rows: every product and sum is exact in float32, so codes and energies equal numpy's float64
    results bit for bit -- which pins the column masks, the tile tails, the ones column and the CSR lookup"""
    N, e = 257, 72
    rng = np.random.RandomState(7)
    ints = lambda *shape: rng.randint(-2, 3, size=shape).astype(np.float32)
    w = {"We": ints(N, e), "be": ints(e), "Wd": ints(e, N), "bd": ints(N),
         "U": rng.randint(-1, 2, size=(U_DOM, K)).astype(np.float32), "V": rng.randint(-1, 2, size=(N, K)).astype(np.float32)}
    urm = H.make_urm(U_DOM, N, 8)
    eng = _ganmf_engine(w, urm)
    for n in (65, 257):
        ids = H.make_ids(U_DOM, n, 9)
        c64, v64 = H.oracle64(w, urm, ids, generated)
        feat, val = eng.discriminate(ids, generated=generated)
        np.testing.assert_array_equal(feat.astype(np.float64), c64)
        np.testing.assert_array_equal(val, v64)
    eng.close()


def test_repeatable_across_calls_and_handles():
    N, e = 257, 72
    w, urm = _ganmf_case(N, e, True)
    ids = H.make_ids(U_DOM, 257, 257)
    a, b = _ganmf_engine(w, urm), _ganmf_engine(w, urm)
    for generated in (False, True):
        f0, v0 = a.discriminate(ids, generated=generated)
        for eng in (a, b):
            f, v = eng.discriminate(ids, generated=generated)
            assert f.tobytes() == f0.tobytes() and v.tobytes() == v0.tobytes()
    a.close(); b.close()


def test_blocks_inside_the_call():
    """n = 257 in blocks of 100 rows: three blocks, the last one ragged"""
    N, e = 257, 72
    w, urm = _ganmf_case(N, e, True)
    eng = _ganmf_engine(w, urm)
    worst = 0.0
    print()
    for generated in (False, True):
        ids, r64, r32 = _refs(N, e, True, 257, generated)
        one = eng.discriminate(ids, generated=generated)
        got = eng.discriminate(ids, generated=generated, block=100)
        worst = max(worst, _check("blocks of 100, generated=%d" % generated, N, got, r64, r32))
        print("blocks of 100, generated=%d: bit-equal to the one-block call: codes %s, energies %s"
              % (generated, np.array_equal(got[0], one[0]), np.array_equal(got[1], one[1])))
        again = eng.discriminate(ids, generated=generated)      # the block size was the call's own
        assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes()
    eng.close()
    assert worst <= 1.0, worst


def _state(eng, tids):
    return [eng.get_tensor(t, s) for t in tids for s in SLOTS] + [eng.adam_powers()]


@pytest.mark.parametrize("model", ["ganmf", "disganmf"])
def test_training_state_does_not_move(model):
    """train_epoch -> discriminate (both sources, both outputs) -> train_epoch == two uninterrupted train_epochs, bit for bit, in
    every parameter, both Adam moments and the beta powers"""
    N, e = 70, 8
    urm = H.make_urm(U_DOM, N, 5)
    if model == "ganmf":
        w, tids = H.ganmf_weights(U_DOM, N, K, e, 5), list(GANMF_IDS.values())
        make = lambda: _ganmf_engine(w, urm)
    else:
        w, tids = H.disganmf_weights(U_DOM, N, K, 2, e, 5), _dis_tids(2)
        make = lambda: _dis_engine(w, urm, "tanh")
    rng = np.random.RandomState(3)
    perms = [rng.permutation(U_DOM), rng.permutation(U_DOM)]
    ids = H.make_ids(U_DOM, 129, 4)
    plain, probed = make(), make()
    losses = []
    for eng in (plain, probed):
        l0 = eng.train_epoch(perms[0])
        if eng is probed:
            for generated in (False, True):
                feat, val = eng.discriminate(ids, generated=generated, block=50)
                assert np.isfinite(feat).all() and np.isfinite(val).all()
        losses.append((l0, eng.train_epoch(perms[1])))
    for a, b in zip(losses[0], losses[1]):
        np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    for a, b in zip(_state(plain, tids), _state(probed, tids)):
        assert a.tobytes() == b.tobytes()
    plain.close(); probed.close()


@pytest.mark.parametrize("m", [2.0, 0.001])
def test_energies_tie_to_the_step_loss(m):
    """d_reg = 0: mean_real + max(0, m mean_real - mean_generated) of a minibatch's energies is the loss the discriminator step on
    those rows reports (GANMF.py:131; tolerance of the loss checks in tests/test_gpu_parity.py); m = 2: hinge on, m = 0.001: off"""
    N, e, B = 257, 72, 64
    w, urm = _ganmf_case(N, e, True)
    eng = _ganmf_engine(w, urm, B=B, hp=dict(HP, m=m))
    uids = np.random.RandomState(2).permutation(U_DOM)[:B].astype(np.int32)
    real = eng.discriminate(uids, features=False)[1]
    gen = eng.discriminate(uids, generated=True, features=False)[1]
    hinge = m * real.mean() - gen.mean()
    want = real.mean() + max(0.0, hinge)
    loss = eng.train_step(0, uids)
    print("\nm=%g: mean_real %.6e mean_generated %.6e hinge %.3e -> %.8e, step loss %.8e" % (m, real.mean(), gen.mean(), hinge, want, loss))
    assert (hinge > 0) == (m == 2.0)
    np.testing.assert_allclose(loss, want, rtol=5e-5, atol=1e-7)
    eng.close()


@pytest.mark.parametrize("generated", [False, True])
def test_low_precision_handle_meets_the_same_bound(generated):
    """a handle that trains in fp16 still answers in the fp32-accurate arithmetic"""
    N, e = 257, 72
    w, urm = _ganmf_case(N, e, True)
    eng = _ganmf_engine(w, urm, mfma="f16")
    ids, r64, r32 = _refs(N, e, True, 257, generated)
    print()
    worst = _check("mfma=f16 handle, generated=%d" % generated, N, eng.discriminate(ids, generated=generated), r64, r32)
    eng.close()
    wd = H.disganmf_weights(U_DOM, 70, K, 2, 8, 28)
    urm_d = H.make_urm(U_DOM, 70, 70)
    eng = _dis_engine(wd, urm_d, "tanh", mfma="f16")
    ids = H.make_ids(U_DOM, 65, 65)
    worst = max(worst, _check("mfma=f16 DisGANMF handle, generated=%d" % generated, 70, eng.discriminate(ids, generated=generated),
                              H.oracle64(wd, urm_d, ids, generated, "tanh"), H.restatement32(wd, urm_d, ids, generated, "tanh"),
                              kinds=("features", "logit")))
    eng.close()
    assert worst <= 1.0, worst


# ---- the classes ---------------------------------------------------------------------------------------------------------------
def _fetched(model):
    return {n: model._get(t) for n, t in GANMF_IDS.items()}


@pytest.mark.parametrize("mode", ["user", "item"])
def test_ganmf_class_methods(mode, golden_dir):
    from ganmf_amd.GANMF import GANMF
    urm = sps.load_npz(os.path.join(golden_dir, "tiny_urm.npz")).tocsr()
    np.random.seed(3)
    model = GANMF(urm, mode=mode, seed=3, is_experiment=True)
    model.fit(num_factors=4, emb_dim=6, epochs=2, batch_size=16, d_lr=1e-3, g_lr=1e-3, m=3, recon_coefficient=0.1)
    w, fit_urm = _fetched(model), model._URM_fit
    n, N = fit_urm.shape
    all_ids = np.arange(n)
    codes = model.autoencoder_codes()
    assert codes.shape == (model.num_users, 6) and codes.dtype == np.float32
    old = np.asarray(fit_urm.dot(w["We"]) + w["be"], dtype=np.float32)      # the host formula this method used to run
    c64, v64 = H.oracle64(w, fit_urm, all_ids, False)
    c32, v32 = H.restatement32(w, fit_urm, all_ids, False)
    print()
    worst = _check("GANMF class %s mode, stored rows" % mode, N, (codes, model.discriminator_energy()), (c64, v64), (c32, v32))
    lim = H.allowed("codes", N, c64, c32)
    print("autoencoder_codes() against the old host formula: %.3e, allowed %.3e, ratio %.3f"
          % (np.abs(codes - old).max(), lim, np.abs(codes - old).max() / lim))
    assert np.abs(codes - old).max() <= lim
    some = np.array([5, 0, 5, n - 1])
    np.testing.assert_array_equal(model.autoencoder_codes(some), codes[some])
    g64, g32 = H.oracle64(w, fit_urm, some, True), H.restatement32(w, fit_urm, some, True)
    worst = max(worst, _check("GANMF class %s mode, generated rows" % mode, N,
                              (model.autoencoder_codes(some, generated=True), model.discriminator_energy(some, generated=True)), g64, g32))
    assert worst <= 1.0, worst
    study = model.discriminator_study()
    assert set(study) == {"energy_real", "energy_generated", "mean_real", "mean_generated", "hinge", "hinge_active"}
    assert study["energy_real"].shape == (n,) and study["energy_generated"].shape == (n,)
    assert study["hinge"] == 3 * study["mean_real"] - study["mean_generated"] and study["hinge_active"] == (study["hinge"] > 0)
    assert model.discriminator_study(some)["energy_real"].shape == (4,)
    model.engine.close()


def test_disganmf_class_methods(golden_dir):
    from ganmf_amd.DisGANMF import DisGANMF
    urm = sps.load_npz(os.path.join(golden_dir, "tiny_urm.npz")).tocsr()
    np.random.seed(4)
    model = DisGANMF(urm, mode="user", seed=4, is_experiment=True)
    model.fit(num_factors=4, d_layers=2, d_nodes=6, d_hidden_act="tanh", epochs=2, batch_size=16, d_lr=1e-3, g_lr=1e-3)
    w = {"W0": model._get(0), "b0": model._get(1), "W1": model._get(2), "b1": model._get(3), "Wo": model._get(4), "bo": model._get(5),
         "U": model._get(100), "V": model._get(101)}
    n, N = urm.shape
    ids = np.arange(n)
    print()
    worst = 0.0
    for generated in (False, True):
        logit, feat = model.discriminator_logits(generated=generated, return_features=True)
        assert logit.shape == (n,) and feat.shape == (n, 6)
        np.testing.assert_array_equal(model.discriminator_logits(generated=generated), logit)
        worst = max(worst, _check("DisGANMF class, generated=%d" % generated, N, (feat, logit),
                                  H.oracle64(w, urm, ids, generated, "tanh"), H.restatement32(w, urm, ids, generated, "tanh"),
                                  kinds=("features", "logit")))
    assert worst <= 1.0, worst
    study = model.discriminator_study([3, 1, 2])
    assert set(study) == {"p_real", "p_generated", "mean_p_real", "mean_p_generated", "accuracy"}
    assert study["p_real"].shape == (3,) and study["p_generated"].shape == (3,) and 0.0 <= study["accuracy"] <= 1.0
    with pytest.raises(AttributeError):
        model.autoencoder_codes()
    model.engine.close()


def test_loaded_checkpoint(golden_dir, tmp_path):
    """loadModel of a bundle that holds the golden checkpoint's tensors (LastFM, item mode, emb_dim 133; the two kernels, which are not
    held as fixtures, drawn here), 2 048 rows against the float64 oracle"""
    from ganmf_amd import tf_bundle as tb
    from ganmf_amd.GANMF import GANMF
    t = np.load(os.path.join(golden_dir, "kat1_checkpoint_tensors.npz"))
    train = sps.load_npz(os.path.join(golden_dir, "LastFM_URM_train.npz")).tocsr()
    n_fit, N, e = 17632, 1884, 133
    drawn = H.ganmf_weights(4, N, 1, e, 12)
    w = {"We": drawn["We"], "be": t["be"], "Wd": drawn["Wd"], "bd": t["bd"], "U": t["U"], "V": t["V"]}
    tb.write_bundle(str(tmp_path / "GANMF_item"), {
        "autoencoder/encoding/kernel": w["We"], "autoencoder/encoding/bias": w["be"], "autoencoder/decoding/kernel": w["Wd"],
        "autoencoder/decoding/bias": w["bd"], "generator/user_embeddings": w["U"], "generator/item_embeddings": w["V"]})
    with open(str(tmp_path / "build_params.pkl"), "wb") as f:
        pickle.dump({"num_factors": 1, "emb_dim": e}, f)
    model = GANMF(train, mode="item", is_experiment=True)
    model.loadModel(str(tmp_path))
    assert model.num_users == n_fit and model.num_items == N
    ids = np.random.RandomState(1).permutation(n_fit)[:2048].astype(np.int32)
    print()
    worst = 0.0
    for generated in (False, True):
        got = (model.autoencoder_codes(ids, generated=generated), model.discriminator_energy(ids, generated=generated))
        worst = max(worst, _check("loaded checkpoint, generated=%d" % generated, N, got,
                                  H.oracle64(w, model._URM_fit, ids, generated), H.restatement32(w, model._URM_fit, ids, generated)))
    study = model.discriminator_study(ids[:64])
    assert study["hinge"] is None and study["hinge_active"] is None and study["energy_real"].shape == (64,)
    model.engine.close()
    assert worst <= 1.0, worst


def test_sharded_model_equals_the_single_engine():
    """dist_backend="local", world_size=3: the master engine answers (it gets the training matrix on first use); after one epoch
    the sharded model's outputs equal the single-engine model's within the bound"""
    from ganmf_amd.GANMF import GANMF
    N, e = 70, 8
    urm = H.make_urm(U_DOM, N, 6)
    w0 = H.ganmf_weights(U_DOM, N, K, e, 6)
    ids = H.make_ids(U_DOM, 129, 7)
    out, weights = {}, {}
    for name, kw in (("single", {}), ("sharded", dict(dist_backend="local", world_size=3))):
        np.random.seed(9)
        model = GANMF(urm, mode="user", seed=1, is_experiment=True, **kw)
        model.initial_weights = w0
        model.fit(num_factors=K, emb_dim=e, epochs=1, batch_size=64, m=2, recon_coefficient=0.05)
        out[name] = [model.engine.discriminate(ids, generated=g) for g in (False, True)]
        weights[name] = _fetched(model)
        model.engine.close()
    assert type(out["sharded"]) is list
    print()
    worst = 0.0
    for gi, generated in enumerate((False, True)):
        r64, r32 = H.oracle64(weights["single"], urm, ids, generated), H.restatement32(weights["single"], urm, ids, generated)
        worst = max(worst, _check("sharded (world 3) against the oracle on its own weights, generated=%d" % generated, N, out["sharded"][gi],
                                  H.oracle64(weights["sharded"], urm, ids, generated), H.restatement32(weights["sharded"], urm, ids, generated)))
        for kind, a, b, r6, r3 in zip(("codes", "energy"), out["sharded"][gi], out["single"][gi], r64, r32):
            dev, lim = H.deviations(a, b, kind == "energy"), H.allowed(kind, N, r6, r3)
            print("sharded against single, generated=%d %s: deviation %.3e, allowed %.3e, ratio %.3f" % (generated, kind, dev, lim, dev / lim))
            worst = max(worst, dev / lim)
    assert worst <= 1.0, worst


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_run_nothing():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    N, e = 70, 8
    w, urm = _ganmf_case(N, e, True)
    eng = _ganmf_engine(w, urm)
    feat, val = eng.discriminate(np.array([], dtype=np.int32))
    assert feat.shape == (0, e) and feat.dtype == np.float32 and val.shape == (0,) and val.dtype == np.float64
    for bad in ([0, U_DOM], [-1], [3, 2 ** 31 - 1]):
        with pytest.raises(L.GanmfError, match="out of range"):
            eng.discriminate(np.array(bad), generated=True)
        ids = np.array(bad, dtype=np.int32)
        out = np.zeros(len(bad), dtype=np.float64)
        rc = eng.lib.ganmf_discriminate(eng.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(bad), 0, None,
                                        out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == -1 and b"out of range" in eng.lib.ganmf_last_error() and not out.any()
    ids = np.array([1, 2], dtype=np.int32)
    assert eng.lib.ganmf_discriminate(eng.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), 2, 0, None, None) == -1
    assert eng.lib.ganmf_last_error()
    with pytest.raises(ValueError):
        eng.discriminate(ids, features=False, value=False)
    # the handle is usable as before
    np.testing.assert_array_equal(eng.discriminate(ids)[0], eng.discriminate(ids, value=False)[0])
    eng.close()
    bare = Engine(U_DOM, N, K, e, 64, **HP)      # no matrix set: stored rows are refused, generated rows are not
    with pytest.raises(L.GanmfError, match="ganmf_set_urm_csr"):
        bare.discriminate(ids)
    assert bare.discriminate(ids, generated=True)[0].shape == (2, e)
    bare.close()
