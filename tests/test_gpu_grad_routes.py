"""Gradients of the fp32-accurate dense step, row by row against the fp64 oracle, on every kernel route the planner takes.

Parameters and losses cannot see how large a gradient is: from zero moments TF-Adam's first update is lr g / (|g| + eps) = +-lr
whatever |g| is, and Adam is invariant to a constant scale of a gradient tensor.  The Adam slots do show it: one step from zero
moments leaves SLOT_ADAM_M = (1 - beta1) g.  So every case below runs one discriminator and one generator step on a fresh handle and
holds gWe, gbe, gWd, gbd (DisGANMF: gW_l, gb_l, gWo, gbo) and gU, gV to GANMFOracle / DisGANMFOracle.d_grads / g_grads in fp64, and
one epoch (d_steps = g_steps = 2, at least four minibatches per pass: pass_stage, the lazy U row flush, staged generator rows) holds
both moments of every tensor to the oracle's optimizer slots.

Rule (one for every route): each row is normalised by its own fp64 |terms| bound (tests/helpers_grad.py), and its ratio
max|got - ref| / max bound must be <= max(2e-5, 2 r32), never above 1e-4, where r32 is the same ratio of the numpy float32 oracle on
that tensor; a row whose bound is 0 (a user outside the batch with g_reg = 0) must match exactly.  The epoch runs at lr = 1e-6, so
the two sides' parameters cannot drift apart by more than 2 lr per update and the moments stay a statement about the arithmetic;
their bounds are composed from the per-step bounds B_t of the oracle run in lockstep (m: sum (1 - b1) b1^(T-t) B_t, v: sum (1 - b2)
b2^(T-t) 2 |g_t| B_t).

Every case names the forms it must take (GANMF_DEBUG_PLAN lines and the one-launch classes of Engine.profile_read(), on a second
handle with profiling on whose moments must equal the first handle's bit for bit).  A case FAILS when a form it names does not
appear: a planner change that moves a shape off its route must pick a new shape, not silently lose coverage.  The dense real path
is forced (GANMF_SPARSE = GANMF_SPARSE_D = 0): tests/test_gpu_sparse_path.py covers the sparse one.

relu is left out of the gradient check: a pre-activation within rounding of 0 flips a unit, and no max-norm bound holds there
(tests/test_gpu_mfma_modes.py::test_disganmf_f16_hidden_layers)."""
import numpy as np
import pytest
import scipy.sparse as sps

from oracle.ganmf_oracle import DisGANMFOracle, GANMFOracle, batch_slices
from tests.helpers_grad import MomentBounds, allowed, d_bounds, forms, g_bounds, grad_from_m, plan_lines, row_ratio

pytestmark = pytest.mark.gpu

GANMF_IDS = {"We": 0, "be": 1, "Wd": 2, "bd": 3, "U": 100, "V": 101}

# name: (U, N, k, e, B, g_reg, forms the single step must take, forms the epoch must take, run the epoch).  Forms as measured on
# the MI355X: "gWd+reduce_dE" (T_GWD_RED) was taken at none of these shapes (the fused-Adam pair launch replaced it); the skinny-N
# stream carries dE (N = e = 32 behind K = 17 632) once 2B x K reaches 4 Mi (gemm_skinny_n_eligible), i.e. at C1 width with B = 128,
# not B = 32; the tiny shapes take bf16x3 kg 4 with stand-alone gWd / gWe (ring 2, kg 1), not an fp32 fallback.
PAIRS = {"front", "gUb+gV pair", "dE+d_coef", "gWd+gWe fused Adam"}
STAGED = {"lazy U rows", "staged pass"}
GANMF_CASES = {
    "c2": (6040, 3706, 250, 992, 128, 0.0, PAIRS | {"decode merged", "bf16x3 kg4", "64x32", "split-K reduce"}, STAGED, True),
    "c2_ragged": (6040, 3706, 250, 992, 100, 0.0, PAIRS | {"decode two-batch", "64x32"}, STAGED, True),
    "c1_lastfm": (1884, 17632, 10, 32, 32, 0.0, {"skinny-K", "f32 kg1", "decode two-batch", "gWd+gWe fused Adam"}, STAGED, True),
    "c1_b128": (1884, 17632, 10, 32, 128, 0.0, {"skinny-N"}, STAGED | {"skinny-N"}, True),
    "staged_gv": (2000, 17632, 128, 256, 128, 0.0, {"gV staged", "decode merged", "f32 kg1", "split-K reduce"}, STAGED, True),
    "c3_item": (10109, 2113, 100, 748, 128, 0.0, PAIRS | {"decode merged", "64x32", "split-K reduce"}, STAGED, True),
    "deep_split": (500, 3706, 16, 64, 8, 0.0, PAIRS | {"split-K reduce", "skinny-K", "decode two-batch"}, STAGED, True),
    "c4_shard": (25000, 50000, 250, 1024, 128, 0.0, {"bf16x3 tile128", "bf16x3 kg4", "gV staged", "d_coef stand-alone",
                                                     "gWd+gWe fused Adam", "split-K reduce"}, set(), False),
    "tiny_a": (5, 63, 1, 1, 8, 0.0, {"front", "gUb+gV pair", "gWd stand-alone", "d_coef stand-alone"}, set(), True),   # (one minibatch)
    "tiny_b": (37, 53, 5, 7, 8, 0.0, {"front", "gUb+gV pair", "gWd stand-alone", "d_coef stand-alone"}, STAGED, True),
    "g_reg": (700, 1100, 20, 64, 32, 1e-3, PAIRS, {"per-step U rows", "staged pass"}, True),
}

# name: (U, N, k, e, B, layers, act, GANMF_TUNE, head form (single step and epoch), other forms of the single step).
# The fp32 discriminator step has two head forms (lib/step_disganmf.inc dis_d_step): with one layer the head rides in the slab-sum
# launch and the output-layer column sums in the layer-0 gradient launch ("D head in slab sum"); with GANMF_TUNE dis_top_gw=0, or
# more than one layer, dis_head_kernel / dis_dz_top_kernel run as a launch of their own ("D head own launch").  dis_uid_grad_kernel
# and GANMF_TUNE dis_uid_top act only in the low-precision modes (uid_apart and uid_top need low_precision): no fp32 route.
DIS_CASES = {
    "c5": (6040, 3706, 250, 1024, 128, 1, "linear", "", {"D head in slab sum"}, {"front", "64x32", "gUb+gV pair"}),
    "c5_dis_top_gw0": (6040, 3706, 250, 1024, 128, 1, "linear", "dis_top_gw=0", {"D head own launch"}, {"front", "64x32", "gUb+gV pair"}),
    "mid_tanh2_b128": (1000, 1500, 64, 192, 128, 2, "tanh", "", {"D head own launch"}, {"front", "64x32", "split-K reduce"}),
    "mid_tanh2_b100": (1000, 1500, 64, 192, 100, 2, "tanh", "", {"D head own launch"}, {"front", "64x32", "split-K reduce"}),
    "mid_sigmoid3_b128": (1000, 1500, 64, 192, 128, 3, "sigmoid", "", {"D head own launch"}, {"front", "64x32", "split-K reduce"}),
    "mid_sigmoid3_b100": (1000, 1500, 64, 192, 100, 3, "sigmoid", "", {"D head own launch"}, {"front", "64x32", "split-K reduce"}),
}

STEP_HP = dict(d_lr=1e-5, g_lr=1e-5, d_reg=1e-3, recon_coefficient=0.3)
EPOCH_HP = dict(d_lr=1e-6, g_lr=1e-6, d_reg=1e-3, recon_coefficient=0.3)


def _urm(rng, U, N, dens):
    """Ratings 1-5 (a kernel that wrote 1 for a stored entry must fail), the last item stored, every user holding a rating."""
    nnz = max(U, int(U * N * dens))
    rows = np.concatenate([np.arange(U), rng.randint(0, U, nnz)])
    cols = np.concatenate([rng.randint(0, N, U), rng.randint(0, N, nnz)])
    rows[0], cols[0] = 0, N - 1
    m = sps.csr_matrix((np.ones(rows.size, np.float32), (rows, cols)), shape=(U, N))
    m.sum_duplicates()
    m.data = rng.randint(1, 6, m.nnz).astype(np.float32)
    m.sort_indices()
    return m


def _oracles(kind, U, N, k, e, hp, layers=1, act="linear", seed=3):
    """fp64 and float32 oracles on the same fp32 parameters; biases away from 0 (so the d_reg term of a bias gradient shows)."""
    rng = np.random.RandomState(seed + 100)
    if kind == "ganmf":
        o = GANMFOracle(U, N, k, e, dtype=np.float64, seed=seed, m=5.0, **hp)
        o.set_params(be=rng.randn(e) * 0.05, bd=rng.randn(N) * 0.05)
        o32 = GANMFOracle(U, N, k, e, dtype=np.float32, seed=seed, m=5.0, **hp)
        ids = dict(GANMF_IDS)
    else:
        o = DisGANMFOracle(U, N, k, d_layers=layers, d_nodes=e, d_hidden_act=act, dtype=np.float64, seed=seed, **hp)
        o.p["W0"][0, :] *= 1.0 / U      # the float(uid) row: logits of order 1
        if act == "tanh":               # pre-activations in tanh's near-linear range: with tanh' at its supremum the bound stays
            for l in range(layers):     # within ~100x of float32's own rounding (glorot weights put it 1e4x above)
                o.p["W%d" % l] *= 0.3
        o.set_params(**{"b%d" % l: rng.randn(e) * 0.05 for l in range(layers)}, bo=rng.randn(1) * 0.05)
        o32 = DisGANMFOracle(U, N, k, d_layers=layers, d_nodes=e, d_hidden_act=act, dtype=np.float32, seed=seed, **hp)
        ids = {n: i for i, n in enumerate(o.D_NAMES)}
        ids.update(U=100, V=101)
    p0 = {n: v.astype(np.float32) for n, v in o.p.items()}
    o.set_params(**p0)
    o32.set_params(**p0)
    return o, o32, p0, ids


def _engine(kind, U, N, k, e, B, hp, urm, p0, ids, layers=1, act="linear", profile=False):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    if kind == "ganmf":
        eng = Engine(U, N, k, e, B, m=5.0, **hp)
    else:
        eng = Engine(U, N, k, e, B, model=L.MODEL_DISGANMF, d_layers=layers, d_act=act, m=0.0, **hp)
    eng.set_urm(urm)
    for n, tid in ids.items():
        eng.set_tensor(tid, p0[n])
    if profile:
        eng.profile(True)
    return eng


def _moments(eng, ids):
    from ganmf_amd import _lib as L
    return {n: (eng.get_tensor(tid, slot=L.SLOT_ADAM_M).copy(), eng.get_tensor(tid, slot=L.SLOT_ADAM_V).copy()) for n, tid in ids.items()}


def _run_both(monkeypatch, capfd, run, make, ids):
    """`run(eng)` on a plain handle and on a profiled one: the moments of both, bit for bit equal, and the forms the runs took."""
    monkeypatch.setenv("GANMF_DEBUG_PLAN", "1")
    monkeypatch.setenv("GANMF_SPARSE", "0")
    monkeypatch.setenv("GANMF_SPARSE_D", "0")
    capfd.readouterr()
    eng = make(False)
    run(eng)
    got = _moments(eng, ids)
    eng.close()
    peng = make(True)
    run(peng)
    prof = peng.profile_read()
    pgot = _moments(peng, ids)
    peng.close()
    for n in got:
        for s in (0, 1):
            np.testing.assert_array_equal(pgot[n][s], got[n][s], err_msg="%s slot %d: profiled handle differs" % (n, s + 1))
    text = capfd.readouterr().err
    plans = plan_lines(text)
    classes = {c["name"]: c["launches"] for c in prof}
    return got, forms(plans, classes), plans, classes


def _schedule_forms(kind, classes, d_steps, g_steps, g_updates):
    """Forms read from launch counts of a run of d_steps discriminator and g_steps generator steps (g_updates of them in generator
    passes of more than one step).  Each is concluded only when the class it counts was recorded at all: a renamed tag or a profiling
    gap leaves the form missing (and the case failing) instead of letting it hold vacuously."""
    seen = set()
    rows_u = classes.get("adam_rows_U", 0)
    if rows_u > 0 and g_updates:
        seen.add("lazy U rows" if rows_u < g_updates else "per-step U rows")       # one advance + one flush per pass
    gen = sum(v for c, v in classes.items() if c.startswith("gemm_generator"))
    if 0 < gen < d_steps + g_steps:
        seen.add("staged pass")         # the generated rows of a discriminator pass formed in front of it
    heads = classes.get("dis_head", 0)
    if kind == "dis" and g_steps > 0 and heads >= g_steps:      # every generator step launches the head once
        if heads == g_steps:
            seen.add("D head in slab sum")
        elif heads == g_steps + d_steps:
            seen.add("D head own launch")
    return seen


class _Report:
    def __init__(self, case):
        self.case, self.rows, self.bad = case, [], []

    def check(self, what, got, ref, bound, got32):
        r, zero_bad = row_ratio(got, ref, bound)
        r32, _ = row_ratio(got32, ref, bound)
        tol = allowed(r32)
        self.rows.append((what, r, r32, tol))
        if r > tol or zero_bad.size:
            self.bad.append((what, r, tol, zero_bad[:8].tolist()))

    def finish(self, seen, expect, plans, classes):
        print("\n[%s] forms: %s" % (self.case, ", ".join(sorted(seen))))
        for p in plans:
            print("   plan %-44s M=%d N=%d K=%d batch=%d tile %d ring %d kg %d nsplit %d %s %s" % (
                p["tag"], p["M"], p["N"], p["K"], p["batch"], p["tile"], p["ring"], p["kg"], p["nsplit"], p["mode"], p["rest"]))
        print("   classes: %s" % ", ".join("%s x%d" % kv for kv in sorted(classes.items())))
        for what, r, r32, tol in self.rows:
            print("   %-12s ratio %.2e  (float32 oracle %.2e, allowed %.2e)" % (what, r, r32, tol))
        assert not self.bad, (self.case, self.bad)
        assert expect <= seen, (self.case, "forms not taken", sorted(expect - seen), "seen", sorted(seen))


# -- single steps -----------------------------------------------------------------------------------------------------------------
def _single_step(kind, case, U, N, k, e, B, hp, layers, act, expect, monkeypatch, capfd):
    rng = np.random.RandomState(sum(map(ord, case)))
    urm = _urm(rng, U, N, 0.02 if U * N < 2e8 else 0.004)
    o, o32, p0, ids = _oracles(kind, U, N, k, e, hp, layers, act)
    uids = rng.choice(U, min(B, U), replace=False)

    def make(profile):
        return _engine(kind, U, N, k, e, B, hp, urm, p0, ids, layers, act, profile)

    def run(eng):
        eng.train_step(0, uids)
        eng.train_step(1, uids)

    got, seen, plans, classes = _run_both(monkeypatch, capfd, run, make, ids)
    seen |= _schedule_forms(kind, classes, 1, 1, 0)
    rep = _Report(case)
    X = urm[uids].toarray().astype(np.float64)
    X32 = X.astype(np.float32)
    _, gd = o.d_grads(uids, X)
    bd = d_bounds(o, uids, X)
    _, gd32 = o32.d_grads(uids, X32)
    for n in o.D_NAMES:
        rep.check("g" + n, grad_from_m(got[n][0]), gd[n], bd[n], gd32[n])
    for oo, g in ((o, gd), (o32, gd32)):       # the discriminator update the generator step reads
        for n in oo.D_NAMES:
            oo.opt_d.apply_dense(n, oo.p[n], g[n])
        oo.opt_d.finish()
        oo.opt_d.slots.clear()
    del gd, bd, gd32
    _, gg = o.g_grads(uids, X)
    bg = g_bounds(o, uids, X)
    _, gg32 = o32.g_grads(uids, X32)
    for n in o.G_NAMES:
        rep.check("g" + n, grad_from_m(got[n][0]), gg[n], bg[n], gg32[n])
    rep.finish(seen, expect, plans, classes)


@pytest.mark.parametrize("case", list(GANMF_CASES))
def test_ganmf_one_step_gradients(case, monkeypatch, capfd):
    """One D step then one G step from zero moments: every gradient row by row (rows of U outside the batch exactly 0 when g_reg = 0;
    the g_reg case gives every row a gradient, and the lazy-row form is not taken)."""
    U, N, k, e, B, g_reg, expect, _, _ = GANMF_CASES[case]
    _single_step("ganmf", case, U, N, k, e, B, dict(STEP_HP, g_reg=g_reg), 1, "linear", expect, monkeypatch, capfd)


@pytest.mark.parametrize("case", list(DIS_CASES))
def test_disganmf_one_step_gradients(case, monkeypatch, capfd):
    U, N, k, e, B, layers, act, tune, head, expect = DIS_CASES[case]
    monkeypatch.setenv("GANMF_TUNE", tune)
    _single_step("dis", case, U, N, k, e, B, dict(STEP_HP, g_reg=0.0), layers, act, head | expect, monkeypatch, capfd)


# -- one epoch: both moments ------------------------------------------------------------------------------------------------------
def _epoch(kind, case, U, N, k, e, B, hp, layers, act, expect, monkeypatch, capfd, d_steps=2, g_steps=2):
    rng = np.random.RandomState(sum(map(ord, case)) + 1)
    urm = _urm(rng, U, N, 0.02)
    o, o32, p0, ids = _oracles(kind, U, N, k, e, hp, layers, act)
    B = min(B, U)
    n = min(U, 4 * B + max(1, B // 2))       # four full minibatches and a ragged one (or every row)
    perm = rng.permutation(U)[:n]
    slices = batch_slices(n, B)

    def make(profile):
        return _engine(kind, U, N, k, e, B, hp, urm, p0, ids, layers, act, profile)

    got, seen, plans, classes = _run_both(monkeypatch, capfd, lambda eng: eng.train_epoch(perm, d_steps, g_steps), make, ids)
    nd, ng = len(slices) * d_steps, len(slices) * g_steps
    seen |= _schedule_forms(kind, classes, nd, ng, ng if len(slices) > 1 else 0)
    mb = MomentBounds()
    for _ in range(d_steps):
        for a, b in slices:
            uids = perm[a:b]
            X = urm[uids].toarray().astype(np.float64)
            _, g = o.d_grads(uids, X)
            bnd = d_bounds(o, uids, X)
            for nm in o.D_NAMES:
                mb.add(nm, g[nm], bnd[nm])
                o.opt_d.apply_dense(nm, o.p[nm], g[nm])
            o.opt_d.finish()
    for _ in range(g_steps):
        for a, b in slices:
            uids = perm[a:b]
            X = urm[uids].toarray().astype(np.float64)
            _, g = o.g_grads(uids, X)
            bnd = g_bounds(o, uids, X)
            for nm in o.G_NAMES:
                mb.add(nm, g[nm], bnd[nm])
            o.opt_g.apply_sparse_all_rows("U", o.p["U"], g["U"])
            o.opt_g.apply_dense("V", o.p["V"], g["V"])
            o.opt_g.finish()
    o32.train_epoch(urm, perm, B, d_steps, g_steps)
    rep = _Report(case + " epoch")
    for nm in ids:
        opt, opt32 = (o.opt_d, o32.opt_d) if nm in o.D_NAMES else (o.opt_g, o32.opt_g)
        for s, bound in ((0, mb.m[nm]), (1, mb.v[nm])):
            rep.check(nm + (".m", ".v")[s], got[nm][s], opt.slots[nm][s], bound, opt32.slots[nm][s])
    rep.finish(seen, expect, plans, classes)


@pytest.mark.parametrize("case", [c for c, v in GANMF_CASES.items() if v[8]])
def test_ganmf_epoch_moments(case, monkeypatch, capfd):
    """One epoch, d_steps = g_steps = 2, four full minibatches and a ragged one per pass: SLOT_ADAM_M and SLOT_ADAM_V of every
    tensor row by row against the oracle's optimizer slots.  (c4_shard: single steps only -- its fp64 epoch would take minutes.)"""
    U, N, k, e, B, g_reg, _, expect, _ = GANMF_CASES[case]
    _epoch("ganmf", case, U, N, k, e, B, dict(EPOCH_HP, g_reg=g_reg), 1, "linear", expect, monkeypatch, capfd)


@pytest.mark.parametrize("case", list(DIS_CASES))
def test_disganmf_epoch_moments(case, monkeypatch, capfd):
    U, N, k, e, B, layers, act, tune, head, _ = DIS_CASES[case]
    monkeypatch.setenv("GANMF_TUNE", tune)
    _epoch("dis", case, U, N, k, e, B, dict(EPOCH_HP, g_reg=0.0), layers, act, STAGED | head, monkeypatch, capfd)
