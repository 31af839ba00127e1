"""CFGAN on the device: the mask sampler against its uint64 restatement and its own statistics, one D-step and one G-step per row
against the float64 restatement, the one-call epoch against the same slices step by step and against float64, and the class
(fit in both modes, device evaluation, early stopping, the Saver bundle, the numpy mask sampler, the refusals).

Shapes: 65 rows (slices of 32, 32 and 1 at batch 32), I = 64 / 70 / 400 (no tail word, tails of 6 and 16 bits), profiles of 0, 1, 63,
64, 65, I - 1 and I items among the first rows (helpers_cfgan.make_case)."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_cfgan as H
from tests.helpers_grad import allowed, grad_from_m, row_ratio

pytestmark = pytest.mark.gpu

ROWS, BATCH = 65, 32
DIS_FACTOR, DIS_FLOOR = 4.0, 5e-5      # test_gpu_trajectory.py: x the float32 restatement's own deviation from float64, or the floor


def _k_rows(urm, ratio):
    from ganmf_amd.CFGAN import mask_size
    return [mask_size(urm.shape[1] - int(n), ratio) for n in np.diff(urm.indptr)]


def _engine(urm, d_nodes=4, g_nodes=4, dl=1, gl=1, d_act="linear", g_act="linear", scheme="ZP", coef=0.0, d_reg=0.0, g_reg=0.0,
            seed=0, k_rows=None, ratio=0.5, lr=1e-3, batch=BATCH):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    eng = Engine(urm.shape[0], urm.shape[1], 1, d_nodes, batch, d_lr=lr, g_lr=lr, d_reg=d_reg, g_reg=g_reg, m=0.0,
                 recon_coefficient=0.0, model=L.MODEL_CFGAN, d_layers=dl, d_act=d_act)
    eng.set_urm(urm)
    eng.cfgan_init(g_nodes, gl, g_act, batch, batch, scheme, coef, seed, _k_rows(urm, ratio) if k_rows is None else k_rows)
    return eng


def _tids(dl, gl):
    from ganmf_amd import _lib as L
    return {"D": list(range(2 * dl + 2)), "G": [L.T_CFGAN_G0 + i for i in range(2 * gl + 2)]}


def _set_state(eng, w, dl, gl):
    """parameters from w, zero moments, fresh beta powers"""
    from ganmf_amd import _lib as L
    for key, ids in _tids(dl, gl).items():
        for tid, a in zip(ids, w[key]):
            eng.set_tensor(tid, a)
            eng.set_tensor(tid, np.zeros_like(a), slot=L.SLOT_ADAM_M)
            eng.set_tensor(tid, np.zeros_like(a), slot=L.SLOT_ADAM_V)
    eng.set_adam_powers([0.9, 0.999, 0.9, 0.999])


def _get(eng, key, dl, gl, slot=0):
    return [eng.get_tensor(t, slot) for t in _tids(dl, gl)[key]]


def _masks(urm, scheme, seed):
    """injected planes: random non-interactions, a plane the scheme does not use left empty"""
    rng = np.random.RandomState(seed)
    free = urm.toarray() == 0
    zr = (rng.rand(*urm.shape) < 0.4) & free if scheme != "PM" else np.zeros(urm.shape, bool)
    pm = (rng.rand(*urm.shape) < 0.4) & free if scheme != "ZR" else np.zeros(urm.shape, bool)
    return zr, pm


def _upload(eng, zr, pm):
    from ganmf_amd.CFGAN import pack_mask_rows
    eng.cfgan_set_masks(pack_mask_rows(zr), pack_mask_rows(pm))


# ---- sampler -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,scheme", [(64, "ZP"), (70, "ZR"), (70, "PM"), (400, "ZP"), (1000, "ZP")])
def test_sampler_planes_equal_the_restatement(I, scheme):
    from ganmf_amd.CFGAN import pack_mask_rows, unpack_mask_rows
    urm = H.make_case(I)
    dense = urm.toarray() != 0
    for ratio in (0.0, 0.05, 0.5, 0.7, 1.0):
        k = _k_rows(urm, ratio)
        for seed in (0, 7):
            eng = _engine(urm, scheme=scheme, seed=seed, k_rows=k)
            seen = {}
            for epoch in (0, 1, 1000, 1):
                eng.cfgan_draw_masks(epoch)
                zr, pm = eng.cfgan_masks()
                want = H.sampler_masks(urm, scheme, k, seed, epoch)
                assert zr.tobytes() == pack_mask_rows(want[0]).tobytes(), (ratio, seed, epoch, "ZR")
                assert pm.tobytes() == pack_mask_rows(want[1]).tobytes(), (ratio, seed, epoch, "PM")
                for plane, used in ((zr, scheme != "PM"), (pm, scheme != "ZR")):
                    bits = unpack_mask_rows(plane, I)
                    assert not (bits & dense).any()
                    assert np.array_equal(bits.sum(axis=1), np.array(k) if used else np.zeros(ROWS, int))
                if epoch in seen:
                    assert seen[epoch] == (zr.tobytes(), pm.tobytes())      # the same (seed, epoch) twice: the same bytes
                seen[epoch] = (zr.tobytes(), pm.tobytes())
            if 0.0 < ratio < 1.0:
                assert len(set(seen.values())) == 3      # different epochs: different bytes
            eng.close()


def test_sampler_statistics_over_2000_epochs():
    """Every eligible column's count within 5 sigma of E k / n (sigma^2 = E p (1 - p)), the mean ZR-PM overlap within 5 sigma of k^2 / n
    (hypergeometric variance).  numpy's own choice() stays below 3.5 sigma on both at these shapes."""
    from ganmf_amd.CFGAN import unpack_mask_rows
    I, E = 400, 2000
    nk = [(69, 20), (64, 32), (5, 2), (399, 39), (100, 90), (337, 10)]
    rng = np.random.RandomState(5)
    dense = np.zeros((len(nk), I), dtype=np.float32)
    for r, (n, k) in enumerate(nk):
        dense[r, rng.choice(I, size=I - n, replace=False)] = 1.0
    urm = sps.csr_matrix(dense)
    eng = _engine(urm, scheme="ZP", seed=3, k_rows=[k for _, k in nk], batch=len(nk))
    counts = np.zeros((2, len(nk), I))
    overlap = np.zeros(len(nk))
    for epoch in range(E):
        eng.cfgan_draw_masks(epoch)
        zr, pm = (unpack_mask_rows(p, I) for p in eng.cfgan_masks())
        counts[0] += zr
        counts[1] += pm
        overlap += (zr & pm).sum(axis=1)
    eng.close()
    worst_c = worst_o = 0.0
    for r, (n, k) in enumerate(nk):
        free = dense[r] == 0
        p = k / n
        sigma = np.sqrt(E * p * (1 - p))
        for plane in range(2):
            assert not counts[plane, r, ~free].any()
            z = np.abs(counts[plane, r, free] - E * p).max() / sigma
            worst_c = max(worst_c, z)
            assert z <= 5.0, ("count", r, plane, z)
        var = k * p * (1 - p) * (n - k) / (n - 1)
        z = abs(overlap[r] / E - k * k / n) / np.sqrt(var / E)
        worst_o = max(worst_o, z)
        assert z <= 5.0, ("overlap", r, z)
    print("sampler statistics: worst column count %.2f sigma, worst mean overlap %.2f sigma" % (worst_c, worst_o))


# ---- steps -------------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(64, 4, 4, 1, 1, "linear", "linear", "ZR", 0.0, 0.0),
              (70, 40, 72, 3, 3, "tanh", "sigmoid", "ZP", 0.01, 0.02),
              (400, 40, 72, 1, 3, "relu", "tanh", "PM", 0.01, 0.0),
              (70, 4, 4, 3, 1, "sigmoid", "relu", "ZP", 0.0, 0.02)]


def _weights(I, dn, gn, dl, gl, seed=1):
    from ganmf_amd.CFGAN import init_weights
    return init_weights(seed, I, dn, dl, gn, gl)


@pytest.mark.parametrize("I,dn,gn,dl,gl,d_act,g_act,scheme,d_reg,g_reg", STEP_CASES)
def test_one_step_per_row_against_float64(I, dn, gn, dl, gl, d_act, g_act, scheme, d_reg, g_reg):
    from ganmf_amd import _lib as L
    urm = H.make_case(I)
    C = urm.toarray()
    zr, pm = _masks(urm, scheme, 2)
    w = _weights(I, dn, gn, dl, gl)
    coef = 0.3
    eng = _engine(urm, dn, gn, dl, gl, d_act, g_act, scheme, coef, d_reg, g_reg)
    _upload(eng, zr, pm)
    kw = dict(d_act=d_act, g_act=g_act, d_reg=d_reg, g_reg=g_reg, zr_coefficient=coef)
    worst = 0.0
    for kind, key in ((0, "D"), (1, "G")):
        for r0, nb in ((0, 32), (32, 32), (64, 1)):
            _set_state(eng, w, dl, gl)
            loss = float(eng.cfgan_step(kind, r0, nb))
            got = [grad_from_m(m) for m in _get(eng, key, dl, gl, L.SLOT_ADAM_M)]
            other = _get(eng, "G" if key == "D" else "D", dl, gl, L.SLOT_ADAM_M)
            assert all(not m.any() for m in other)      # Adam updates this step's variables only
            sl = slice(r0, r0 + nb)
            c, M, Z = C[sl], C[sl] + pm[sl], zr[sl].astype(np.float64)
            r64, r32 = H.CFGANRef(w, **kw), H.CFGANRef(w, dtype=np.float32, **kw)
            if kind == 0:
                (l64, g64), (l32, g32), bounds = r64.d_grads(c, M), r32.d_grads(c, M), H.abs_d_bounds(r64, c, M)
            else:
                (l64, g64), (l32, g32), bounds = r64.g_grads(c, M, Z), r32.g_grads(c, M, Z), H.abs_g_bounds(r64, c, M, Z)
            dev32 = abs(float(l32) - float(l64))
            assert abs(loss - float(l64)) <= max(4.0 * dev32, 1e-5 * abs(float(l64))), (key, r0, loss, float(l64), dev32)
            for i, (g, ref, g32_, b) in enumerate(zip(got, g64, g32, bounds)):
                ratio, bad = row_ratio(g, ref, b)
                base, _ = row_ratio(g32_, ref, b)
                worst = max(worst, ratio)
                assert bad.size == 0, (key, r0, i, "rows with bound 0 differ", bad[:8])
                assert ratio <= allowed(base), (key, r0, i, ratio, base)
    eng.close()
    print("step gradients, largest row ratio: %.3g" % worst)


# ---- epoch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,dn,gn,dl,gl,d_act,g_act,scheme,d_reg,g_reg", STEP_CASES[1:3])
def test_epoch_equals_its_steps_and_float64(I, dn, gn, dl, gl, d_act, g_act, scheme, d_reg, g_reg):
    urm = H.make_case(I)
    C = urm.toarray()
    w = _weights(I, dn, gn, dl, gl)
    coef = 0.3
    engines = [_engine(urm, dn, gn, dl, gl, d_act, g_act, scheme, coef, d_reg, g_reg) for _ in range(2)]
    kw = dict(d_act=d_act, g_act=g_act, d_reg=d_reg, g_reg=g_reg, zr_coefficient=coef, d_lr=1e-3, g_lr=1e-3)
    r64, r32 = H.CFGANRef(w, **kw), H.CFGANRef(w, dtype=np.float32, **kw)
    for eng in engines:
        _set_state(eng, w, dl, gl)
    slices = [(0, 32), (32, 32), (64, 1)]
    losses = {"got": [], "f64": [], "f32": []}
    for epoch in range(3):
        zr, pm = _masks(urm, scheme, 10 + epoch)
        for eng in engines:
            _upload(eng, zr, pm)
        dlo, glo = engines[0].cfgan_epoch(epoch, 2, 2, draw=False)
        by_step = [engines[1].cfgan_step(kind, r0, nb) for kind in (0, 1) for _ in range(2) for r0, nb in slices]
        assert np.concatenate([dlo, glo]).tobytes() == np.array(by_step, dtype=np.float32).tobytes()
        losses["got"].append(np.concatenate([dlo, glo]).astype(np.float64))
        for name, ref in (("f64", r64), ("f32", r32)):
            losses[name].append(np.concatenate(ref.epoch(C, pm, zr, 2, 2, BATCH, BATCH)).astype(np.float64))
    errs, base = {}, {}
    for key in ("D", "G"):
        a, b = (_get(eng, key, dl, gl) for eng in engines)
        for i, (x, y, p64, p32) in enumerate(zip(a, b, r64.p[key], r32.p[key])):
            assert x.tobytes() == y.tobytes(), (key, i)
            scale = np.abs(p64).max()
            errs["%s%d" % (key, i)] = np.abs(x.reshape(p64.shape) - p64).max() / scale
            base["%s%d" % (key, i)] = np.abs(p32.astype(np.float64) - p64).max() / scale
    ids = np.arange(ROWS)
    s = engines[0].scores(ids)
    assert s.tobytes() == engines[1].scores(ids).tobytes()
    s64, s32 = r64.scores(C), r32.scores(C)
    errs["scores"] = np.abs(s - s64).max() / np.abs(s64).max()
    base["scores"] = np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max()
    for name, n in (("dloss", slice(0, 6)), ("gloss", slice(6, 12))):
        f64 = np.concatenate([l[n] for l in losses["f64"]])
        errs[name] = np.abs(np.concatenate([l[n] for l in losses["got"]]) - f64).max() / np.abs(f64).max()
        base[name] = np.abs(np.concatenate([l[n] for l in losses["f32"]]) - f64).max() / np.abs(f64).max()
    for eng in engines:
        eng.close()
    print("CFGAN epoch (I=%d, %s/%s): " % (I, d_act, g_act) + ", ".join("%s %.2g (f32 %.2g)" % (n, errs[n], base[n]) for n in sorted(errs)))
    for n, v in errs.items():
        assert v <= max(DIS_FACTOR * base[n], DIS_FLOOR), (n, v, base[n])


# ---- class -------------------------------------------------------------------------------------------------------------------------
FIT = dict(d_nodes=8, g_nodes=12, d_layers=2, g_layers=2, d_hidden_act="tanh", g_hidden_act="sigmoid", d_lr=1e-3, g_lr=1e-3,
           d_reg=0.01, g_reg=0.01, d_steps=1, g_steps=2, d_batch_size=32, g_batch_size=16, zr_ratio=0.7, zp_ratio=0.1, zr_coefficient=0.2)


@pytest.mark.parametrize("mode,scheme", [("user", "ZP"), ("item", "PM")])
def test_fit_scores_equal_the_restatement(mode, scheme):
    from ganmf_amd.CFGAN import CFGAN, draw_masks_numpy, init_weights, pack_mask_rows
    urm = H.make_case(70)
    model = CFGAN(urm, mode=mode, seed=4, is_experiment=True, mask_sampler="numpy")
    np.random.seed(21)
    assert model.fit(epochs=2, scheme=scheme, allow_worse=None, **FIT) == 3
    fitm = model._URM_fit
    rows, I = fitm.shape
    w = init_weights(4, I, 8, 2, 12, 2)
    kw = dict(d_act="tanh", g_act="sigmoid", d_lr=1e-3, g_lr=1e-3, d_reg=0.01, g_reg=0.01, zr_coefficient=0.2)
    r64, r32 = H.CFGANRef(w, **kw), H.CFGANRef(w, dtype=np.float32, **kw)
    C = fitm.toarray()
    np.random.seed(21)
    for _ in range(2):
        zr, pm = draw_masks_numpy(fitm, scheme, 0.7)
        for ref in (r64, r32):
            ref.epoch(C, pm, zr, 1, 2, 32, 16)
    got_zr, got_pm = model.engine.cfgan_masks()      # the last epoch's planes are exactly draw_masks_numpy's
    assert got_zr.tobytes() == pack_mask_rows(zr).tobytes() and got_pm.tobytes() == pack_mask_rows(pm).tobytes()
    s64, s32 = r64.scores(C), r32.scores(C)
    if mode == "item":
        s64, s32 = s64.T, s32.T
    users = np.arange(urm.shape[0])
    got = model._compute_item_score(users)
    assert got.shape == urm.shape
    err = np.abs(got - s64).max() / np.abs(s64).max()
    base = np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max()
    print("CFGAN fit %s: scores %.2g (f32 %.2g)" % (mode, err, base))
    assert err <= max(DIS_FACTOR * base, DIS_FLOOR)
    sub = np.array([5, 0, 64, 5])
    assert got[sub].tobytes() == model._compute_item_score(sub).tobytes()
    assert model.URM_train.shape == urm.shape
    model.engine.close()


@pytest.fixture(scope="module")
def fitted():
    from ganmf_amd.CFGAN import CFGAN
    urm = H.make_case(70, seed=3)
    model = CFGAN(urm, seed=9, is_experiment=True)
    model.fit(epochs=2, scheme="ZP", allow_worse=None, **FIT)
    rng = np.random.RandomState(31)
    t = ((rng.rand(*urm.shape) < 0.15) & (urm.toarray() == 0)) * rng.randint(1, 6, size=urm.shape)
    yield model, urm, sps.csr_matrix(t.astype(np.float32))
    model.engine.close()


@pytest.mark.parametrize("full", [False, True])
def test_device_evaluation_equals_the_host_evaluator(fitted, full):
    from ganmf_amd.base import BaseRecommender
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    model, urm, test = fitted

    class Twin(BaseRecommender):
        def _compute_item_score(self, user_id_array, items_to_compute=None):
            return model._compute_item_score(user_id_array).astype(np.float64)
    cut = [1, 5, 10]
    ev = EvaluatorHoldoutFast(test, cut, full_metrics=full)
    assert ev.use_device_metrics
    dev, _ = ev.evaluateRecommender(model)
    host, _ = EvaluatorHoldoutFast(test, cut, full_metrics=full).evaluateRecommender(Twin(urm))
    for c in cut:
        assert set(dev[c]) == set(host[c])
        for name, v in host[c].items():
            if name == "RMSE" and not full:
                assert np.isnan(dev[c][name]) and np.isnan(v)
                continue
            assert abs(dev[c][name] - v) <= (1e-5 if name == "RMSE" else 1e-12) * max(1.0, abs(v)), (c, name, dev[c][name], v)
    items = model.recommend(np.arange(8), cutoff=5)
    seen = urm.toarray() != 0
    assert all(not seen[u, i] for u in range(8) for i in items[u])


def test_early_stopping_restores_every_tensor():
    from ganmf_amd.CFGAN import CFGAN

    class Watch(object):
        def __init__(self):
            self.values, self.states = [0.5, 0.4, 0.3, 0.9], []

        def evaluateRecommender(self, m):
            self.states.append([m.sess.run(r) for r in m.params['D'] + m.params['G']])
            return {5: {"MAP": self.values[len(self.states) - 1]}}, ""
    urm = H.make_case(70, seed=3)
    model = CFGAN(urm, seed=9, is_experiment=True)
    watch = Watch()
    assert model.fit(epochs=10, scheme="ZP", allow_worse=1, freq=1, validation_evaluator=watch, **FIT) == 3
    assert len(watch.states) == 3
    now = [model.sess.run(r) for r in model.params['D'] + model.params['G']]
    assert len(now) == 12
    for a, best, last in zip(now, watch.states[0], watch.states[2]):
        assert a.tobytes() == best.tobytes() and a.tobytes() != last.tobytes()
    model.engine.close()


def test_bundle_names_and_round_trip(fitted, tmp_path):
    from ganmf_amd.CFGAN import CFGAN
    from ganmf_amd.tf_bundle import read_bundle
    model, urm, _ = fitted
    model.saveModel(str(tmp_path), "cfgan_ckpt")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cfgan_ckpt.data-00000-of-00001", "cfgan_ckpt.index"]
    data = read_bundle(str(tmp_path / "cfgan_ckpt"))
    want = {}
    for l in range(2):
        want["discriminator/D_hidden_%d/kernel" % l] = (140 if l == 0 else 8, 8)
        want["discriminator/D_hidden_%d/bias" % l] = (8,)
        want["generator/G_hidden_%d/kernel" % l] = (70 if l == 0 else 12, 12)
        want["generator/G_hidden_%d/bias" % l] = (12,)
    want.update({"discriminator/D_output/kernel": (8, 1), "discriminator/D_output/bias": (1,),
                 "generator/G_output/kernel": (12, 70), "generator/G_output/bias": (70,)})
    assert {k: v.shape for k, v in data.items()} == want
    assert [r.name for r in model.params['D']][:2] == ["discriminator/D_hidden_0/kernel", "discriminator/D_hidden_0/bias"]
    twin = CFGAN(urm, is_experiment=True)
    twin.load_bundle(str(tmp_path), "cfgan_ckpt", d_hidden_act="tanh", g_hidden_act="sigmoid")
    ids = np.arange(urm.shape[0])
    assert twin._compute_item_score(ids).tobytes() == model._compute_item_score(ids).tobytes()
    twin.engine.close()


def test_wrong_model_entries_refuse():
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    urm = H.make_case(70)
    eng = _engine(urm)
    ids = np.arange(4, dtype=np.int32)
    calls = [lambda: eng.train_epoch(np.arange(ROWS)), lambda: eng.train_step(0, ids), lambda: eng.discriminate(ids),
             lambda: eng.als_half_sweep(0, 0.1), lambda: eng.pure_svd(np.zeros((65, 4), np.float32), 1),
             lambda: eng.itemknn_fit(L.ITEMKNN_PRODUCT, 5), lambda: eng.slim_bpr_init(), lambda: eng.comm_init_local(1),
             lambda: eng.recommend_candidates(ids, 3), lambda: eng.bench_scores(4),
             lambda: eng.cfgan_init(4, 1, "linear", 32, 32, "ZR", 0.0, 0, np.zeros(ROWS)), lambda: eng.cfgan_step(0, 60, 32),
             lambda: eng.cfgan_step(2, 0, 4), lambda: eng.get_tensor(L.T_USER_EMB), lambda: eng.get_tensor(L.T_CFGAN_G0 + 4)]
    for i, call in enumerate(calls):      # the first ten are other models' entries: the message names this one
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_CFGAN" if i < 10 else None):
            call()
    assert eng.get_tensor(L.T_CFGAN_G0 + 3).shape == (1, 70) and eng.get_tensor(0).shape == (140, 4)
    eng.close()
    other = Engine(ROWS, 70, 2, 4, 32)
    for call in (lambda: other.cfgan_draw_masks(0), lambda: other.cfgan_step(0, 0, 4), lambda: other.cfgan_masks()):
        with pytest.raises(L.GanmfError, match="GANMF_MODEL_CFGAN"):
            call()
    other.close()
    with pytest.raises(L.GanmfError, match="single-GPU"):
        Engine(ROWS, 70, 1, 4, 32, model=L.MODEL_CFGAN, world_size=2)
    with pytest.raises(L.GanmfError, match="fp32-accurate"):
        Engine(ROWS, 70, 1, 4, 32, model=L.MODEL_CFGAN, mfma="bf16")
