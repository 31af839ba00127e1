"""Warm-start state: every slot of every tensor and the four Adam powers, written through the ABI, resumed from, and held to fp64.

Every other training test starts from a fresh handle (zero moments, the initial beta powers).  Here the handle's training state is
written from outside -- ganmf_set_tensor on SLOT_ADAM_M / SLOT_ADAM_V / SLOT_BEST, ganmf_set_adam_powers -- and the claim under test
is the one include/ganmf_hip.h makes: PARAM + ADAM_M + ADAM_V of every tensor + the four powers are the WHOLE training state of a
single-GPU handle.

1. test_slot_round_trip: shapes far from every padding multiple; a pattern that encodes (tensor, slot, flat index) exactly in fp32 is
   uploaded to every (tensor, slot), and only after all uploads is everything read back, bit for bit (slot-to-slot, segment and pad
   aliasing of lib/abi_core.inc copy_view); snapshot_best / restore_best move PARAM <-> BEST only; the powers round-trip in the order
   {b1p_D, b2p_D, b1p_G, b2p_G} (a D step advances the first pair only); one D and one G step from that state stay finite.
2. test_exported_run_resumes_bit_for_bit: engine A trains 3 epochs with an odd number of generator steps in each (item_embeddings
   ends in its second buffer), one of them over a permutation that leaves a third of the rows out; PARAM, M, V and the powers are
   exported.  "fresh": a new engine given that state, "self": an engine that re-uploads its own exported state mid-run; both then run
   2 epochs of d_steps = g_steps = 2 and must give A's losses, tensors, moments, powers and scores (both orientations) bit for bit.
   Every case names the forms it must take and FAILS when one does not appear (tests/test_gpu_grad_routes.py).
3. test_warm_step_updates / test_warm_epoch_moments: a warm state built on the host -- Glorot-style parameters, v = s^2 with s
   log-uniform over S_RANGE (v over 2 x as many decades), m = s u with u uniform in +-M_OVER_S (both signs, |m| / sqrt(v) within
   what Adam itself reaches, (1 - b1) / sqrt(1 - b2) = 3.16), 5 % of the elements with m = v = 0 exactly, beta powers as after t
   optimizer steps (t differs between D and G: T_PAIRS) -- loaded into the engine and into the fp64 and float32 oracles.
   (a) one D and one G step at lr = 1e-3: per tensor the update delta = theta_after - theta_before (fp64 from the fp32 values),
       r = max|delta - delta_ref| / (max|delta_ref| + 2^-24 max|theta|) <= allowed(r32); elements with m = v = 0 and no gradient
       (rows of U outside the batch, g_reg = 0) keep theta, m and v exactly.
   (b) one epoch, d_steps = g_steps = 2, lr = 1e-6 (EPOCH_HP): both moments row by row (row_ratio / allowed, MomentBounds seeded with
       |m0|, |v0|), step losses against fp64 at rtol 2e-4, atol 1e-7.
   The float32 oracle must itself be within 2e-5 of fp64 on every tensor (asserted: the 1e-4 cap of `allowed` never decides).
4. test_restore_best_mid_training: one epoch, snapshot_best, two epochs, restore_best, one epoch; the oracles do the same with
   set_params(best) while their optimizer slots and powers run on (the reference's load_model restores parameters only).  Moments and
   losses of the last epoch as in 3(b); a twin engine rebuilt from (BEST as PARAM, exported M, V, powers) gives the last epoch bit
   for bit.

Why S_RANGE = (1e-6, 1e-2), i.e. v in [1e-12, 1e-4]: gradients here are 1e-7 .. 1e-3, so the range spans state-dominated elements
(s >> |g|), gradient-dominated ones and the eps regime (sqrt(v) below 1e-4, where sqrt(v + eps) and sqrt(v) + eps part).  The
lower end is where the update's sensitivity to the rounding of g, alpha (1 - b1) / sqrt(v), stays below the rule: at s = 1e-6 a
gradient error of 1e-7 x its |terms| bound (<= 1e-3) moves the update by 1e-5 alpha.

Measured (largest ratio over the tensors of a case and over t; r32 = float32 oracle on the CPU; the gpu columns are not measured
yet -- every test prints its ratios as _Report does, fill them from the first MI355X run):

    case          (a) r32    (a) gpu    (b) r32    (b) gpu
    ganmf_pairs   1.4e-05   -          6.2e-07   -
    ganmf_g_reg   1.4e-05   -          8.4e-07   -
    dis_tanh2     1.5e-05   -          5.6e-07   -
    dis_linear1   1.5e-05   -          5.0e-07   -
"""
import types

import numpy as np
import pytest

from oracle.ganmf_oracle import GANMFOracle, batch_slices
from tests.helpers_grad import (MomentBounds, adam_powers_after, allowed, d_bounds, forms, g_bounds, plan_lines, set_state,
                                urm_paths)
from tests.test_gpu_grad_routes import EPOCH_HP, GANMF_IDS, _oracles, _Report, _schedule_forms, _urm

pytestmark = pytest.mark.gpu

SLOT_NAMES = ("p", "m", "v")                # SLOT_PARAM, SLOT_ADAM_M, SLOT_ADAM_V = 0, 1, 2; SLOT_BEST = 3
DENSE = {"GANMF_SPARSE": "0", "GANMF_SPARSE_D": "0"}
SPARSE_GD = {"GANMF_SPARSE": "1", "GANMF_SPARSE_D": "1"}
REAL_HP = dict(d_lr=1e-4, g_lr=2e-4, d_reg=1e-3, recon_coefficient=0.3)
WARM_STEP_HP = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-3, recon_coefficient=0.3)

# name: how the configuration is built, and the forms its resumed epochs must take
CASES = {
    "ganmf_pairs": dict(build="routes", kind="ganmf", shape=(700, 1100, 20, 64, 32), g_reg=0.0, env=DENSE,
                        forms={"front", "gUb+gV pair", "gWd+gWe fused Adam", "staged pass", "lazy U rows"}),
    "ganmf_g_reg": dict(build="routes", kind="ganmf", shape=(700, 1100, 20, 64, 32), g_reg=1e-3, env=DENSE, forms={"per-step U rows"}),
    "ganmf_sparse_gd": dict(build="sparse", env=SPARSE_GD, forms={"sparse_g", "sparse_d"}),       # the CSC walk and the CSR epilogues
    "dis_tanh2": dict(build="routes", kind="dis", shape=(900, 1100, 64, 128, 64), g_reg=0.0, layers=2, act="tanh", env=DENSE,
                      forms={"D head own launch"}),
    "dis_linear1": dict(build="routes", kind="dis", shape=(900, 1100, 64, 128, 64), g_reg=0.0, layers=1, act="linear", env=DENSE,
                        forms={"D head in slab sum"}),
    "ganmf_f16": dict(build="lp", seed=0, mfma="f16", env={}, forms=set()),        # resume bit-identity only: no accuracy statement
    "dis_bf16": dict(build="lp", seed=3, mfma="bf16", env={}, forms=set()),
    "forced_collectives": dict(build="coll", env=dict(DENSE, GANMF_FORCE_COLLECTIVES="1"), forms={"world_size 1"}),
}
ORACLE_CASES = ("ganmf_pairs", "ganmf_g_reg", "dis_tanh2", "dis_linear1")

S_RANGE = (1e-6, 1e-2)          # sqrt(v) log-uniform over these (module docstring)
M_OVER_S = 3.0
COND = 1e-5                     # how much of alpha the float32 rounding of a gradient may move an update (_warm_state)
T_PAIRS = {0: (0, 7), 7: (7, 5000), 5000: (5000, 0)}        # t of the case -> optimizer steps behind (D, G)


# -- configurations ---------------------------------------------------------------------------------------------------------------
def _dis_ids(layers):
    ids = {}
    for l in range(layers):
        ids["W%d" % l], ids["b%d" % l] = 2 * l, 2 * l + 1
    ids.update({"Wo": 2 * layers, "bo": 2 * layers + 1, "U": 100, "V": 101})
    return ids


def _setup(case, lr_hp=REAL_HP):
    """The configuration of a case: sizes, hyper-parameters, URM, fp32 parameters, tensor ids (nothing of it touches the GPU)."""
    spec = CASES[case]
    c = types.SimpleNamespace(case=case, layers=1, act="linear", mfma=spec.get("mfma"), coll=False, env=spec["env"], m=0.0,
                              expect=spec["forms"])
    rng = np.random.RandomState(sum(map(ord, case)))
    if spec["build"] == "routes":
        c.kind, (c.U, c.N, c.k, c.e, c.B) = spec["kind"], spec["shape"]
        c.layers, c.act = spec.get("layers", 1), spec.get("act", "linear")
        c.hp = dict(lr_hp, g_reg=spec["g_reg"])
        c.m = 5.0 if c.kind == "ganmf" else 0.0
        c.urm = _urm(rng, c.U, c.N, 0.02)
        c.oracles = lambda: _oracles(c.kind, c.U, c.N, c.k, c.e, c.hp, c.layers, c.act)[:2]
        _, _, c.p0, c.ids = _oracles(c.kind, c.U, c.N, c.k, c.e, c.hp, c.layers, c.act)
    elif spec["build"] == "sparse":         # tests/test_gpu_sparse_path.py::test_one_step_gradients_row_by_row, e = 37
        from tests.test_gpu_sparse_path import _rated_urm
        c.kind, (c.U, c.N, c.k, c.e, c.B), c.m = "ganmf", (60, 2300, 9, 37, 40), 5.0
        rng = np.random.RandomState(c.e)
        c.urm = _rated_urm(rng, c.U, c.N, 0.02, "ratings", long_row=True)
        c.hp = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-3, g_reg=0.0, recon_coefficient=0.3)
        o = GANMFOracle(c.U, c.N, c.k, c.e, dtype=np.float64, seed=9, m=c.m, **c.hp)
        o.set_params(be=rng.randn(c.e) * 0.01, bd=rng.randn(c.N) * 0.01)
        c.p0, c.ids = {n: v.astype(np.float32) for n, v in o.p.items()}, dict(GANMF_IDS)
    elif spec["build"] == "lp":             # tests/test_gpu_engine_fuzz.py::test_low_precision_launch_forms_random_config, same draws
        import scipy.sparse as sps
        seed = spec["seed"]
        rng = np.random.RandomState(3000 + seed)
        dis = seed % 4 >= 2
        assert c.mfma == ("f16" if seed % 2 == 0 else "bf16")
        c.U, c.N = int(rng.randint(300, 900)), int(rng.randint(600, 4000))
        c.k, c.e, c.B = int(rng.choice([16, 64, 100, 250])), int(rng.choice([64, 200, 512, 1024])), int(rng.choice([64, 96, 128]))
        c.hp = dict(d_lr=1e-4, g_lr=2e-4, d_reg=float(rng.choice([0.0, 1e-4])), g_reg=0.0, recon_coefficient=float(rng.uniform(0.05, 0.9)))
        c.urm = sps.csr_matrix((rng.rand(c.U, c.N) < 0.04).astype(np.float32))
        U, N, k, e = c.U, c.N, c.k, c.e
        if dis:
            w = {"W0": rng.randn(N + 1, e) * 0.03, "b0": rng.randn(e) * 0.01, "Wo": rng.randn(e, 1) * 0.1, "bo": np.zeros(1),
                 "U": rng.randn(U, k) * 0.1, "V": rng.randn(N, k) * 0.1}
            w["W0"][0, :] *= 1.0 / U        # the float(uid) row
            c.kind, c.ids, c.act = "dis", _dis_ids(1), str(rng.choice(["linear", "tanh", "relu"]))
        else:
            w = {"We": rng.randn(N, e) * 0.03, "be": rng.randn(e) * 0.01, "Wd": rng.randn(e, N) * 0.03, "bd": rng.randn(N) * 0.01,
                 "U": rng.randn(U, k) * 0.1, "V": rng.randn(N, k) * 0.1}
            c.kind, c.ids, c.m = "ganmf", dict(GANMF_IDS), 10.0
        c.p0 = {n: v.astype(np.float32) for n, v in w.items()}
    else:                                   # tests/test_gpu_parity.py::test_rccl_path_single_rank_matches_plain, "small", forced collectives
        from tests.test_gpu_parity import HP, _rand_urm
        c.kind, (c.U, c.N, c.k, c.e, c.B), c.coll = "ganmf", (150, 210, 9, 17, 32), True
        rng = np.random.RandomState(5)
        c.urm = _rand_urm(rng, c.U, c.N, 0.08)
        c.hp = {n: v for n, v in HP.items() if n != "m"}
        c.m = HP["m"]
        o = GANMFOracle(c.U, c.N, c.k, c.e, seed=4, m=c.m, **c.hp)
        c.p0, c.ids = {n: v.astype(np.float32) for n, v in o.p.items()}, dict(GANMF_IDS)
    c.B = min(c.B, c.U)
    return c


def _env(monkeypatch, c):
    monkeypatch.setenv("GANMF_DEBUG_PLAN", "1")
    monkeypatch.delenv("GANMF_TUNE", raising=False)
    for var in ("GANMF_SPARSE", "GANMF_SPARSE_D", "GANMF_FORCE_COLLECTIVES"):
        if var in c.env:
            monkeypatch.setenv(var, c.env[var])
        else:
            monkeypatch.delenv(var, raising=False)


def _engine(c, params=None):
    """A handle of the case with its URM (and its one-rank communicator); `params`: name -> array uploaded to SLOT_PARAM."""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine, comm_unique_id
    kw = dict(c.hp, m=c.m, mfma=c.mfma)
    if c.kind == "dis":
        kw.update(model=L.MODEL_DISGANMF, d_layers=c.layers, d_act=c.act)
    if c.coll:
        kw.update(world_size=1, rank=0)
    eng = Engine(c.U, c.N, c.k, c.e, c.B, **kw)
    eng.set_urm(c.urm)
    if c.coll:
        eng.comm_init(comm_unique_id())
    for n, a in (params or {}).items():
        eng.set_tensor(c.ids[n], a)
    return eng


def _export(eng, ids):
    """PARAM, ADAM_M, ADAM_V of every tensor and the four powers: what the ABI names as the training state"""
    st = {s: {n: eng.get_tensor(tid, slot=i).copy() for n, tid in ids.items()} for i, s in enumerate(SLOT_NAMES)}
    st["powers"] = eng.adam_powers().copy()
    return st


def _load(eng, ids, st):
    for i, s in enumerate(SLOT_NAMES):
        for n, tid in ids.items():
            eng.set_tensor(tid, st[s][n], slot=i)
    eng.set_adam_powers(st["powers"])


def _final(eng, c):
    out = _export(eng, c.ids)
    out["scores"] = eng.scores(np.arange(min(c.U, 64)))
    out["scores_T"] = eng.scores(np.arange(min(c.N, 64)), transposed=True)
    return out


def _assert_same_state(got, ref, what):
    for s in SLOT_NAMES:
        for n in ref[s]:
            np.testing.assert_array_equal(got[s][n], ref[s][n], err_msg="%s: %s slot %s" % (what, n, s))
    for key in ("powers", "scores", "scores_T"):
        if key in ref:
            np.testing.assert_array_equal(got[key], ref[key], err_msg="%s: %s" % (what, key))


def _train(eng, c, perm, d_steps, g_steps):
    if c.coll:
        steps = -(-perm.size // c.B)
        rows = np.minimum(c.B, perm.size - np.arange(steps) * c.B).astype(np.int32)
        dl, gl = eng.train_epoch(perm, d_steps, g_steps, steps_per_pass=steps, global_batch_rows=rows)
    else:
        dl, gl = eng.train_epoch(perm, d_steps, g_steps)
    return np.array(dl), np.array(gl)


def _forms_seen(c, eng, text, d_counts, g_counts, lazy_g):
    """forms of a profiled run of d_counts / g_counts steps (lazy_g of the generator steps in passes of more than one step)"""
    plans = plan_lines(text)
    classes = {p["name"]: p["launches"] for p in eng.profile_read()}
    seen = forms(plans, classes) | _schedule_forms(c.kind, classes, d_counts, g_counts, lazy_g)
    paths = urm_paths(text)
    if paths and all(p[0] for p in paths):
        seen.add("sparse_g")
    if paths and all(p[1] for p in paths):
        seen.add("sparse_d")
    if eng.comm_info() == (1, 0):
        seen.add("world_size 1")
    return seen, plans, classes


# -- 1: slot round trip -----------------------------------------------------------------------------------------------------------
def _pattern(t_index, slot, shape):
    """(tensor, slot, flat index) as an integer below 2^15 times 2^-16: exact in fp32, every value of the handle distinct in
    magnitude, below 1/4; alternating signs except for SLOT_ADAM_V (v >= 0)."""
    n = int(np.prod(shape))
    assert n < 512 and t_index < 8
    a = ((((t_index * 4 + slot) << 9) + 1 + np.arange(n)).astype(np.float32) * np.float32(2.0 ** -16))
    if slot != 2:
        a[1::2] *= -1
    return a.reshape(shape)


@pytest.mark.parametrize("model", ["ganmf", "disganmf"])
def test_slot_round_trip(model):
    """GANMF (37, 53, 5, 7, 8) and DisGANMF with d_layers = 2, d_nodes = 7: the [N+1, e] layer-0 kernel with its float(uid) row (two
    segments), [e, e], the [e, 1] output kernel stored as one row, [1], biases as rows of the extended kernels, ldk / lde pads."""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    U, N, k, e, B = 37, 53, 5, 7, 8
    rng = np.random.RandomState(1)
    urm = _urm(rng, U, N, 0.1)
    hp = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-3, recon_coefficient=0.3)
    if model == "ganmf":
        eng, ids = Engine(U, N, k, e, B, m=5.0, **hp), dict(GANMF_IDS)
        shapes = {"We": (N, e), "be": (1, e), "Wd": (e, N), "bd": (1, N), "U": (U, k), "V": (N, k)}
    else:
        eng, ids = Engine(U, N, k, e, B, model=L.MODEL_DISGANMF, d_layers=2, d_act="tanh", m=0.0, **hp), _dis_ids(2)
        shapes = {"W0": (N + 1, e), "b0": (1, e), "W1": (e, e), "b1": (1, e), "Wo": (e, 1), "bo": (1, 1), "U": (U, k), "V": (N, k)}
    eng.set_urm(urm)
    names = list(ids)
    for n in names:
        assert eng.shape(ids[n]) == shapes[n], n
    pat = {(n, s): _pattern(i, s, shapes[n]) for i, n in enumerate(names) for s in range(4)}

    def read():
        return {(n, s): eng.get_tensor(ids[n], slot=s).copy() for n in names for s in range(4)}

    def same(got, want, what):
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s slot %d" % (what, key[0], key[1]))

    for s in (3, 1, 0, 2):                       # every upload first ...
        for n in (reversed(names) if s & 1 else names):
            eng.set_tensor(ids[n], pat[(n, s)], slot=s)
    powers = np.array([0.9 ** 3, 0.999 ** 3, 0.9 ** 11, 0.999 ** 11], np.float32)
    eng.set_adam_powers(powers)
    same(read(), pat, "after all uploads")       # ... then every read
    np.testing.assert_array_equal(eng.adam_powers(), powers)
    eng.snapshot_best()
    want = dict(pat)
    want.update({(n, 3): pat[(n, 0)] for n in names})
    same(read(), want, "snapshot_best")
    for n in names:                              # PARAM overwritten with what BEST held before
        eng.set_tensor(ids[n], pat[(n, 3)])
    eng.restore_best()
    same(read(), want, "restore_best")
    np.testing.assert_array_equal(eng.adam_powers(), powers)
    uids = rng.choice(U, B, replace=False)
    b1, b2 = np.float32(0.9), np.float32(0.999)
    ld = eng.train_step(0, uids)
    np.testing.assert_array_equal(eng.adam_powers(), np.array([powers[0] * b1, powers[1] * b2, powers[2], powers[3]], np.float32))
    lg = eng.train_step(1, uids)
    np.testing.assert_array_equal(eng.adam_powers(), np.array([powers[0] * b1, powers[1] * b2, powers[2] * b1, powers[3] * b2], np.float32))
    assert np.isfinite(ld) and np.isfinite(lg), (ld, lg)
    after = read()
    for key, a in after.items():
        assert np.all(np.isfinite(a)), key
        if key[1] == 3:
            np.testing.assert_array_equal(a, want[key], err_msg="BEST moved by a step: %s" % key[0])
    moved = [n for n in names if not np.array_equal(after[(n, 0)], want[(n, 0)])]
    assert moved == names, ("every tensor takes its update", moved)
    assert np.all(np.isfinite(eng.scores(np.arange(U)))) and np.all(np.isfinite(eng.scores(np.arange(N), transposed=True)))
    eng.close()


# -- 2: an exported run resumes bit for bit ---------------------------------------------------------------------------------------
def _odd_rows(n, B):
    """at most n rows, in an odd number of minibatches of B, the last one ragged"""
    nb = -(-n // B)
    if nb % 2 == 1:
        return n
    return max(1, (nb - 1) * B - B // 4)


def _resume_perms(c):
    """Three epochs of one D and one G pass, an odd number of minibatches each (an odd number of generator steps in all), the second
    over a permutation that leaves a third of the rows out; then two epochs of two passes each, the second leaving a third out."""
    prng = np.random.RandomState(5)
    first = [prng.permutation(c.U)[:_odd_rows(n, c.B)] for n in (c.U, c.U - c.U // 3, c.U)]
    assert all((-(-p.size // c.B)) % 2 == 1 for p in first)
    second = [prng.permutation(c.U), prng.permutation(c.U)[:c.U - c.U // 3]]
    return first, second


_RUN_A = {}         # case -> (state exported after the first phase, losses of the second phase, final state): computed once, shared


def _reference_run(c, first, second):
    eng = _engine(c, c.p0)
    for perm in first:
        _train(eng, c, perm, 1, 1)
    mid = _export(eng, c.ids)
    eng.scores(np.arange(min(c.U, 64)))                      # (fills the scoring path's cached operand copy: it must not outlive training)
    eng.scores(np.arange(min(c.N, 64)), transposed=True)
    losses = [_train(eng, c, perm, 2, 2) for perm in second]
    final = _final(eng, c)
    eng.close()
    return mid, losses, final


@pytest.mark.parametrize("variant", ["fresh", "self"])
@pytest.mark.parametrize("case", list(CASES))
def test_exported_run_resumes_bit_for_bit(case, variant, monkeypatch, capfd):
    c = _setup(case)
    _env(monkeypatch, c)
    first, second = _resume_perms(c)
    if case not in _RUN_A:
        _RUN_A[case] = _reference_run(c, first, second)
    mid, ref_losses, ref_final = _RUN_A[case]
    assert not np.array_equal(mid["p"]["V"], c.p0["V"]) and np.any(mid["v"]["U"] != 0)
    capfd.readouterr()
    if variant == "fresh":
        eng = _engine(c)
        _load(eng, c.ids, mid)
    else:
        eng = _engine(c, c.p0)
        for perm in first:
            _train(eng, c, perm, 1, 1)
        own = _export(eng, c.ids)
        _assert_same_state(own, mid, "the first phase repeats")
        _load(eng, c.ids, own)                   # a no-op for the trajectory
    eng.profile(True)
    losses = [_train(eng, c, perm, 2, 2) for perm in second]
    slices = [-(-p.size // c.B) for p in second]
    seen, plans, classes = _forms_seen(c, eng, capfd.readouterr().err, 2 * sum(slices), 2 * sum(slices),
                                       2 * sum(s for s in slices if s > 1))
    final = _final(eng, c)
    eng.close()
    print("\n[%s %s] forms: %s" % (case, variant, ", ".join(sorted(seen))))
    print("   classes: %s" % ", ".join("%s x%d" % kv for kv in sorted(classes.items())))
    for ep, ((dl, gl), (dr, gr)) in enumerate(zip(losses, ref_losses)):
        np.testing.assert_array_equal(dl, dr, err_msg="%s %s: D losses of resumed epoch %d" % (case, variant, ep))
        np.testing.assert_array_equal(gl, gr, err_msg="%s %s: G losses of resumed epoch %d" % (case, variant, ep))
    _assert_same_state(final, ref_final, "%s %s" % (case, variant))
    assert c.expect <= seen, (case, "forms not taken", sorted(c.expect - seen), "seen", sorted(seen))


# -- 3: warm state against the fp64 oracle ----------------------------------------------------------------------------------------
def _warm_state(c, t, cond=None):
    """fp32 host state: the case's parameters, m / v as the module docstring describes, powers after T_PAIRS[t] steps.
    cond: name -> (g, bound), the fp64 gradient the next step will see and its |terms| bound.  A float32 gradient is off by about
    dg = 2^-23 bound, and the update alpha ((1 - b1) g + b1 m) / (sqrt((1 - b2) g^2 + b2 v) + eps) must not amplify that beyond
    COND alpha: sqrt(v) >= (1 - b1) dg / COND, and an element is left at m = v = 0 only where g = 0 exactly or
    (sqrt(1 - b2) |g| + eps)^2 >= (1 - b1) eps dg / COND (below that TF-Adam's first update is a smoothed sign(g): no fp32
    gradient decides it).  The draws are the same with and without cond."""
    rng = np.random.RandomState(sum(map(ord, c.case)) + t)
    st = {"p": dict(c.p0), "m": {}, "v": {}, "zero": {}}
    lo, hi = np.log10(S_RANGE[0]), np.log10(S_RANGE[1])
    for n, a in c.p0.items():
        s = 10.0 ** rng.uniform(lo, hi, a.shape)
        u = rng.uniform(-M_OVER_S, M_OVER_S, a.shape)
        zero = rng.rand(*a.shape) < 0.05
        if cond and n in cond:
            g, dg = np.abs(cond[n][0]).reshape(a.shape), 2.0 ** -23 * np.asarray(cond[n][1]).reshape(a.shape)
            s = np.maximum(s, 0.1 * dg / COND)
            zero &= (g == 0) | ((np.sqrt(1e-3) * g + 1e-8) ** 2 >= 0.1 * 1e-8 * dg / COND)
        m, v = (s * u).astype(np.float32), (s * s).astype(np.float32)
        m[zero], v[zero] = 0.0, 0.0
        st["m"][n], st["v"][n], st["zero"][n] = m, v, zero
    td, tg = T_PAIRS[t]
    st["powers"] = np.array(adam_powers_after(td) + adam_powers_after(tg), np.float32)
    assert st["powers"][0] != st["powers"][2] and st["powers"][1] != st["powers"][3]
    return st


def _loaded_oracles(c, st):
    o, o32 = c.oracles()
    for oo in (o, o32):
        set_state(oo, st["p"], st["m"], st["v"], st["powers"])
    return o, o32


def _step_reference(case, t):
    """(a) on the host: the fp64 oracle's update of every tensor after one D and one G step from the warm state, and the float32
    oracle's ratio r32 against it.  Returns (c, state, uids, before (fp64), delta_ref, r32)."""
    c = _setup(case, WARM_STEP_HP)
    uids = np.random.RandomState(t + 1).choice(c.U, c.B, replace=False)
    X = c.urm[uids].toarray()
    probe = c.oracles()[0]                  # the gradients and |terms| bounds the two steps will see, for _warm_state's condition
    X64 = X.astype(np.float64)
    gd, bd = probe.d_grads(uids, X64)[1], d_bounds(probe, uids, X64)
    cond = {n: (gd[n], bd[n]) for n in probe.D_NAMES}
    st = _warm_state(c, t, cond)
    set_state(probe, st["p"], st["m"], st["v"], st["powers"])
    probe.d_step(uids, X64)
    gg, bg = probe.g_grads(uids, X64)[1], g_bounds(probe, uids, X64)
    cond.update({n: (gg[n], bg[n]) for n in probe.G_NAMES})
    st = _warm_state(c, t, cond)
    assert st["zero"]["U"].mean() >= 0.03         # (5 % drawn everywhere; what the condition leaves differs by tensor, U keeps the rows outside the batch)
    before = {n: a.astype(np.float64) for n, a in c.p0.items()}
    deltas = []
    for oo in _loaded_oracles(c, st):
        oo.d_step(uids, X)
        oo.g_step(uids, X)
        deltas.append({n: np.asarray(oo.p[n], np.float64) - before[n] for n in c.ids})
    r32 = {n: _delta_ratio(deltas[1][n], deltas[0][n], before[n]) for n in c.ids}
    return c, st, uids, before, deltas[0], r32


def _delta_ratio(delta, delta_ref, before):
    return float(np.max(np.abs(delta - delta_ref)) / (np.max(np.abs(delta_ref)) + 2.0 ** -24 * np.max(np.abs(before))))


@pytest.mark.parametrize("t", list(T_PAIRS))
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_warm_step_updates(case, t, monkeypatch, capfd):
    c, st, uids, before, dref, r32 = _step_reference(case, t)
    _env(monkeypatch, c)
    capfd.readouterr()
    eng = _engine(c)
    _load(eng, c.ids, st)
    eng.profile(True)
    eng.train_step(0, uids)
    eng.train_step(1, uids)
    seen, plans, classes = _forms_seen(c, eng, capfd.readouterr().err, 1, 1, 0)
    got = _export(eng, c.ids)
    eng.close()
    rep = _Report("%s t=%d warm step" % (case, t))
    for n in c.ids:
        r = _delta_ratio(got["p"][n].astype(np.float64).reshape(before[n].shape) - before[n], dref[n], before[n])
        tol = allowed(r32[n])
        rep.rows.append(("d" + n, r, r32[n], tol))
        if r > tol or r32[n] > 2e-5:
            rep.bad.append(("d" + n, r, tol, "r32 %.2e" % r32[n]))
    if c.hp["g_reg"] == 0.0:          # m = v = 0 and no gradient: rows of U outside the batch
        still = st["zero"]["U"].copy()
        still[uids] = False
        assert still.sum() > 100
        for s in SLOT_NAMES:
            np.testing.assert_array_equal(got[s]["U"][still], st[s]["U"][still], err_msg="U slot %s where m = v = 0 and g = 0" % s)
    np.testing.assert_array_equal(got["powers"], st["powers"] * np.array([0.9, 0.999, 0.9, 0.999], np.float32))
    step_forms = c.expect & {"front", "gUb+gV pair", "gWd+gWe fused Adam", "D head own launch", "D head in slab sum"}
    rep.finish(seen, step_forms, plans, classes)


def _lockstep_epoch(o, urm, perm, B, d_steps, g_steps, mb):
    """GANMFOracle.train_epoch with the |terms| bound of every step's gradient composed into `mb`"""
    dl, gl = [], []
    slices = batch_slices(len(perm), B)
    for _ in range(d_steps):
        for a, b in slices:
            uids = perm[a:b]
            X = urm[uids].toarray().astype(np.float64)
            loss, g = o.d_grads(uids, X)
            bnd = d_bounds(o, uids, X)
            for nm in o.D_NAMES:
                mb.add(nm, g[nm], bnd[nm])
                o.opt_d.apply_dense(nm, o.p[nm], g[nm])
            o.opt_d.finish()
            dl.append(loss)
    for _ in range(g_steps):
        for a, b in slices:
            uids = perm[a:b]
            X = urm[uids].toarray().astype(np.float64)
            loss, g = o.g_grads(uids, X)
            bnd = g_bounds(o, uids, X)
            for nm in o.G_NAMES:
                mb.add(nm, g[nm], bnd[nm])
            o.opt_g.apply_sparse_all_rows("U", o.p["U"], g["U"])
            o.opt_g.apply_dense("V", o.p["V"], g["V"])
            o.opt_g.finish()
            gl.append(loss)
    return np.array(dl), np.array(gl)


def _epoch_perm(c, rng):
    return rng.permutation(c.U)[:min(c.U, 4 * c.B + max(1, c.B // 2))]      # four full minibatches and a ragged one


def _epoch_reference(case, t):
    """(b) on the host: (c, state, perm, fp64 oracle after the epoch, float32 oracle after it, bounds, fp64 losses)"""
    c = _setup(case, EPOCH_HP)
    st = _warm_state(c, t)
    perm = _epoch_perm(c, np.random.RandomState(t + 2))
    o, o32 = _loaded_oracles(c, st)
    shaped = {s: {n: st[s][n].reshape(o.p[n].shape) for n in c.ids} for s in ("m", "v")}
    mb = MomentBounds(shaped["m"], shaped["v"])
    losses = _lockstep_epoch(o, c.urm, perm, c.B, 2, 2, mb)
    o32.train_epoch(c.urm, perm, c.B, 2, 2)
    return c, st, perm, o, o32, mb, losses


def _check_moments(rep, c, got, o, o32, mb):
    """both moments of every tensor row by row; the float32 oracle itself within 2e-5 (the cap of `allowed` never decides)"""
    for nm in c.ids:
        opt, opt32 = (o.opt_d, o32.opt_d) if nm in o.D_NAMES else (o.opt_g, o32.opt_g)
        for s, bound in ((0, mb.m[nm]), (1, mb.v[nm])):
            what = nm + (".m", ".v")[s]
            rep.check(what, got[SLOT_NAMES[s + 1]][nm], opt.slots[nm][s], bound, opt32.slots[nm][s])
            if rep.rows[-1][2] > 2e-5:
                rep.bad.append((what, "float32 oracle ratio %.2e above 2e-5" % rep.rows[-1][2]))


@pytest.mark.parametrize("t", list(T_PAIRS))
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_warm_epoch_moments(case, t, monkeypatch, capfd):
    c, st, perm, o, o32, mb, (dl_ref, gl_ref) = _epoch_reference(case, t)
    _env(monkeypatch, c)
    capfd.readouterr()
    eng = _engine(c)
    _load(eng, c.ids, st)
    eng.profile(True)
    dl, gl = _train(eng, c, perm, 2, 2)
    nsl = len(batch_slices(len(perm), c.B))
    seen, plans, classes = _forms_seen(c, eng, capfd.readouterr().err, 2 * nsl, 2 * nsl, 2 * nsl)
    got = _export(eng, c.ids)
    eng.close()
    rep = _Report("%s t=%d warm epoch" % (case, t))
    _check_moments(rep, c, got, o, o32, mb)
    np.testing.assert_allclose(dl, dl_ref, rtol=2e-4, atol=1e-7, err_msg="D losses")
    np.testing.assert_allclose(gl, gl_ref, rtol=2e-4, atol=1e-7, err_msg="G losses")
    rep.finish(seen, c.expect, plans, classes)


# -- 4: restore_best in the middle of training ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ganmf_pairs", "dis_tanh2"])
def test_restore_best_mid_training(case, monkeypatch, capfd):
    c = _setup(case, EPOCH_HP)
    _env(monkeypatch, c)
    rng = np.random.RandomState(17)
    perms = [_epoch_perm(c, rng) for _ in range(4)]
    o, o32 = c.oracles()
    mb = MomentBounds()
    best = None
    for ep, perm in enumerate(perms):
        if ep == 3:
            o.set_params(**best[0])
            o32.set_params(**best[1])
        dl_ref, gl_ref = _lockstep_epoch(o, c.urm, perm, c.B, 2, 2, mb)
        o32.train_epoch(c.urm, perm, c.B, 2, 2)
        if ep == 0:
            best = (o.get_params(), o32.get_params())
    capfd.readouterr()
    eng = _engine(c, c.p0)
    _train(eng, c, perms[0], 2, 2)
    eng.snapshot_best()
    at_best = _export(eng, c.ids)
    _train(eng, c, perms[1], 2, 2)
    _train(eng, c, perms[2], 2, 2)
    before = _export(eng, c.ids)
    eng.restore_best()
    after = _export(eng, c.ids)
    for n in c.ids:
        assert not np.array_equal(before["p"][n], at_best["p"][n]), n
    _assert_same_state(after, dict(before, p=at_best["p"]), "restore_best: parameters back, moments and powers as they were")
    twin = _engine(c)
    _load(twin, c.ids, dict(after, p={n: eng.get_tensor(tid, slot=3) for n, tid in c.ids.items()}))
    eng.profile(True)
    dl, gl = _train(eng, c, perms[3], 2, 2)
    dl_t, gl_t = _train(twin, c, perms[3], 2, 2)
    nsl = len(batch_slices(len(perms[3]), c.B))
    seen, plans, classes = _forms_seen(c, eng, capfd.readouterr().err, 2 * nsl, 2 * nsl, 2 * nsl)
    got, got_t = _final(eng, c), _final(twin, c)
    eng.close()
    twin.close()
    np.testing.assert_array_equal(dl_t, dl, err_msg="twin: D losses")
    np.testing.assert_array_equal(gl_t, gl, err_msg="twin: G losses")
    _assert_same_state(got_t, got, "twin rebuilt from (BEST, M, V, powers)")
    rep = _Report("%s restore_best" % case)
    _check_moments(rep, c, got, o, o32, mb)
    np.testing.assert_allclose(dl, dl_ref, rtol=2e-4, atol=1e-7, err_msg="D losses")
    np.testing.assert_allclose(gl, gl_ref, rtol=2e-4, atol=1e-7, err_msg="G losses")
    rep.finish(seen, c.expect, plans, classes)
