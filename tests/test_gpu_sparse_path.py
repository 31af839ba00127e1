"""The sparse real path (sparse_front_kernel, csr_quad in the decode epilogue, csc_rows_kernel and the sp_rows share
of gWe's epilogue) against the fp64 oracle away from the one matrix test_gpu_configs.py::test_c1_sparse_real_path runs: random shapes
and weights, emb_dim beyond one 256-float4 column chunk and off a multiple of 4, empty CSC columns, the last item beside the bias row,
rows of thousands of entries, batches below CSC_BIAS_PARTS, d_steps / g_steps > 1, explicit id lists, partial permutations, the
loopback data-parallel step with ranks left without rows and shards on either side of the planner's density threshold.  Every URM
here holds non-binary values (ratings or play counts): a kernel that wrote 1 for a stored entry would pass every binary matrix.
The paths are forced with GANMF_SPARSE / GANMF_SPARSE_D (read at each ganmf_set_urm_csr) and every case asserts, from the
GANMF_DEBUG_PLAN line of the upload, that the path it asked for is the path that ran."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.dist import shard_bounds
from oracle.ganmf_oracle import DisGANMFOracle, GANMFOracle
from tests.helpers_grad import _abs_d_bounds, _abs_g_bounds, _rowwise
from tests.test_gpu_dist_local import _run_ranks
from tests.test_gpu_multi_launch import _run_staged

pytestmark = pytest.mark.gpu

NAME2ID = {"We": 0, "be": 1, "Wd": 2, "bd": 3, "U": 100, "V": 101}
MODES = {"dense": ("0", None), "sparse_g": ("1", "0"), "sparse_gd": ("1", "1")}
_PLAN = re.compile(r"\[ganmf urm\] set_urm_csr .*-> sparse_g (\d) sparse_d (\d)")


def _err(got, ref):
    return np.max(np.abs(np.asarray(got, np.float64).reshape(np.shape(ref)) - ref)) / (np.max(np.abs(ref)) + 1e-30)


def _set_mode(monkeypatch, mode):
    monkeypatch.setenv("GANMF_DEBUG_PLAN", "1")
    for var, val in zip(("GANMF_SPARSE", "GANMF_SPARSE_D"), MODES[mode] if mode else (None, None)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def _paths(capfd):
    """(sparse_g, sparse_d) of every ganmf_set_urm_csr since the last call, from the GANMF_DEBUG_PLAN lines"""
    return [(int(a), int(b)) for a, b in _PLAN.findall(capfd.readouterr().err)]


def _expect(mode):
    return {"dense": (0, 0), "sparse_g": (1, 0), "sparse_gd": (1, 1)}[mode]


def _values(rng, n, kind):
    if kind == "ratings":
        return rng.randint(1, 6, n).astype(np.float32)
    return np.ceil(rng.lognormal(1.0, 1.0, n)).astype(np.float32)      # play counts: 1 .. ~100


def _rated_urm(rng, U, N, dens, kind, long_row=False):
    """Cold rows, empty columns, the column N - 1 stored, optionally one row of more than 2 000 entries; non-binary values."""
    m = rng.rand(U, N) < dens
    empty = rng.rand(N) < 0.1
    empty[N - 1] = False
    if long_row:
        live = np.flatnonzero(~empty)
        m[0, rng.choice(live, min(live.size, 2001 + rng.randint(0, 200)), replace=False)] = True
    m[:, empty] = False
    m[min(1, U - 1), N - 1] = True
    cold = rng.rand(U) < 0.15
    cold[:min(2, U - 1)] = False
    cold[U - 1] = U > 2
    m[cold] = False
    vals = np.zeros((U, N), np.float32)
    vals[m] = _values(rng, int(m.sum()), kind)
    return sps.csr_matrix(vals)


def _upload_raw(eng, urm):
    """ganmf_set_urm_csr with the arrays exactly as the scipy matrix stores them (Engine.set_urm makes them canonical first)."""
    from ganmf_amd import _lib as L
    indptr = np.ascontiguousarray(urm.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(urm.indices, dtype=np.int32)
    data = np.ascontiguousarray(urm.data, dtype=np.float32)
    L.check(eng.lib.ganmf_set_urm_csr(eng.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                      data.ctypes.data_as(C.POINTER(C.c_float)), urm.shape[0], urm.shape[1]), "ganmf_set_urm_csr")


def _state(eng, ids):
    from ganmf_amd import _lib as L
    out = {n: eng.get_tensor(tid).copy() for n, tid in ids.items()}
    out.update({n + ".m": eng.get_tensor(tid, slot=L.SLOT_ADAM_M).copy() for n, tid in ids.items()})
    out.update({n + ".v": eng.get_tensor(tid, slot=L.SLOT_ADAM_V).copy() for n, tid in ids.items()})
    return out


# -- 1: raw, non-canonical CSR through the C ABI ---------------------------------------------------------------------------------
def _non_canonical(rng, U, N):
    """A rated matrix stored with reversed rows, (r, c) entries split in two stored entries (1.0 + 2.0) and explicit zeros."""
    base = _rated_urm(rng, U, N, 0.12, "ratings")
    indptr, indices, data = [0], [], []
    for r in range(U):
        cols = list(base.indices[base.indptr[r]:base.indptr[r + 1]])
        vals = list(base.data[base.indptr[r]:base.indptr[r + 1]])
        if r % 3 == 0:                                     # reversed column order
            cols, vals = cols[::-1], vals[::-1]
        if r % 4 == 1 and cols:                            # one entry split into 1.0 + 2.0, the second copy last in the row
            vals[0] = 1.0
            cols.append(cols[0]); vals.append(2.0)
        if r % 5 == 2:                                     # stored zeros at columns the row does not hold
            free = np.setdiff1d(np.arange(N), cols)
            for c in rng.choice(free, min(2, free.size), replace=False):
                cols.append(int(c)); vals.append(0.0)
        indices += cols; data += vals
        indptr.append(len(indices))
    raw = sps.csr_matrix((np.array(data, np.float32), np.array(indices, np.int32), np.array(indptr, np.int64)), shape=(U, N))
    can = raw.copy()
    can.sum_duplicates()
    can.sort_indices()
    assert not raw.has_sorted_indices and can.nnz < raw.nnz and np.any(can.data == 0) and np.any(can.data == 3.0)
    assert np.array_equal(raw.toarray(), can.toarray())     # the reference's toarray() sums the duplicates
    return raw, can


@pytest.mark.parametrize("mode", list(MODES))
def test_raw_non_canonical_csr_equals_canonical_upload(mode, monkeypatch, capfd):
    """ganmf_set_urm_csr takes any scipy CSR, as the reference does (INTEGRATION.md passes URM_train.tocsr() as it comes): rows
    in reversed column order, a (row, column) stored twice, explicit zeros.  One D + G epoch from the raw arrays must equal, bit for
    bit, the same epoch from csr.sum_duplicates(); sort_indices() on a fresh handle (losses, parameters, both moments), and both the
    fp64 oracle on the summed matrix.  (Without the host-side canonical form densify_rows lets one duplicate win a store race and
    csr_quad's binary search misses entries of an unsorted row.)"""
    from ganmf_amd.engine import Engine
    U, N, k, e, B = 48, 150, 7, 37, 16
    rng = np.random.RandomState(71)
    raw, can = _non_canonical(rng, U, N)
    hp = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-4, g_reg=1e-5, m=5.0, recon_coefficient=0.3)
    o = GANMFOracle(U, N, k, e, dtype=np.float64, seed=5, **hp)
    o.set_params(be=rng.randn(e) * 0.01, bd=rng.randn(N) * 0.01)
    p0 = o.get_params()
    perm = rng.permutation(U)
    dl_ref, gl_ref = o.train_epoch(can, perm, B, 1, 1)
    _set_mode(monkeypatch, mode)
    capfd.readouterr()
    runs = []
    for canonical in (False, True):
        eng = Engine(U, N, k, e, B, **hp)
        if canonical:
            eng.set_urm(can)
        else:
            _upload_raw(eng, raw)
        for n, tid in NAME2ID.items():
            eng.set_tensor(tid, p0[n])
        dl, gl = eng.train_epoch(perm, 1, 1)
        runs.append((dl, gl, _state(eng, NAME2ID)))
        eng.close()
    (dl, gl, got), (dl_c, gl_c, ref) = runs
    np.testing.assert_array_equal(dl, dl_c, err_msg="D losses, raw vs canonical upload (%s)" % mode)
    np.testing.assert_array_equal(gl, gl_c, err_msg="G losses, raw vs canonical upload (%s)" % mode)
    for n in ref:
        np.testing.assert_array_equal(got[n], ref[n], err_msg="%s, raw vs canonical upload (%s)" % (n, mode))
    for dd, gg, st in runs:
        np.testing.assert_allclose(dd, dl_ref, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(gg, gl_ref, rtol=1e-4, atol=1e-7)
        for n in NAME2ID:
            assert _err(st[n], o.p[n]) <= 1e-4, (mode, n)
    assert _paths(capfd) == [_expect(mode)] * 2


# -- 2: random configurations on the forced sparse path -------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_sparse_random_config(seed, monkeypatch, capfd):
    """Two epochs of a random configuration on the forced sparse path (seeds 0-5: generator only, 6-11: generator + discriminator)
    against the fp64 oracle at the engine fuzz tolerances, and the same seed on the dense path: the sparse run's error may be at most
    twice the dense run's (+1e-6), so a sparse-kernel fault cannot hide inside a tolerance sized for the dense path.  emb_dim runs
    through 1, 3 (one partial float4), 33, 255, 1030 (c4n = 258: a second column chunk of both sparse kernels); batches of 1, 7, 15
    (< CSC_BIAS_PARTS), 64 and more than U; every third seed holds a row of more than 2 000 entries.
    Bounds: a matrix with a row of 2 000 ratings or play counts is ill-conditioned for two epochs of Adam -- the same arithmetic
    evaluated in float32 by the numpy oracle is itself up to 4e-2 (normalised) away from fp64 on such seeds, so no fp32 kernel can be
    held to 2e-4 there.  Each run is therefore held to max(2e-4, 2 x the float32 oracle's error) -- 2e-4 wherever float32 arithmetic
    meets it.  Where it does (every tensor of the float32 oracle within 2e-4), the sparse run is also held to 2 x the larger error of
    the two other fp32 evaluations, the dense run and the float32 oracle, + 1e-6: fp32 evaluations of one trajectory differ in their
    rounding only (measured: sparse 9.6e-6, dense 2.9e-6, float32 oracle 1.4e-5 on one tensor -- one fp32 run can be luckier than
    another), and a sparse-kernel fault (a dropped value, a wrong item row) moves a tensor by orders of magnitude more.  Where float32
    arithmetic does not meet 2e-4, two fp32 trajectories of the same updates drift
    apart by rounding alone (measured: sparse 8.4e-5 against dense 1.1e-5 and float32 oracle 4.0e-5 on one tensor), so that ratio says
    nothing about the kernels; the long rows' arithmetic is held per step instead, row by row, by test_one_step_gradients_row_by_row."""
    from ganmf_amd.engine import Engine
    rng = np.random.RandomState(5000 + seed)
    mode = "sparse_g" if seed < 6 else "sparse_gd"
    e = [1, 3, 33, 255, 1030, int(rng.randint(2, 140))][seed % 6]
    long_row = seed % 3 == 0
    N = int(rng.randint(2300, 3000)) if long_row else int(rng.randint(2, 700))
    U = int(rng.randint(3, 70)) if e >= 255 else int(rng.randint(3, 300))
    B = [1, 7, 15, 64, U + 5][seed % 5]
    k = int(rng.randint(1, 70))
    hp = dict(d_lr=float(10 ** rng.uniform(-4, -2.5)), g_lr=float(10 ** rng.uniform(-4, -2.5)),
              d_reg=float(rng.choice([0.0, 1e-4, 1e-2])), g_reg=float(rng.choice([0.0, 1e-3])),
              m=float(rng.choice([0.001, 1.0, 10.0])), recon_coefficient=float(rng.uniform(0, 1)))
    d_steps, g_steps = int(rng.randint(1, 4)), int(rng.randint(1, 4))
    urm = _rated_urm(rng, U, N, float(rng.choice([0.003, 0.02, 0.08])), "ratings" if seed % 2 == 0 else "plays", long_row)
    if long_row:
        assert np.diff(urm.indptr).max() > 2000
    what = str((mode, U, N, k, e, B, d_steps, g_steps, hp))
    o = GANMFOracle(U, N, k, e, dtype=np.float64, seed=seed, **hp)
    o.set_params(be=rng.randn(e) * 0.01, bd=rng.randn(N) * 0.01)
    p0 = o.get_params()
    perms = [rng.permutation(U) for _ in range(2)]
    o32 = GANMFOracle(U, N, k, e, dtype=np.float32, seed=seed, **hp)
    o32.set_params(**p0)
    refs = [o.train_epoch(urm, p, min(B, U), d_steps, g_steps) for p in perms]
    refs32 = [o32.train_epoch(urm, p, min(B, U), d_steps, g_steps) for p in perms]
    fp32 = {n: _err(o32.p[n], o.p[n]) for n in NAME2ID}
    ltol = max(2e-4, 2.0 * max(np.max(np.abs(a - r) / np.abs(r)) for got, ref in zip(refs32, refs) for a, r in zip(got, ref)))
    errs, losses = {}, {}
    capfd.readouterr()
    for run in (mode, "dense"):
        _set_mode(monkeypatch, run)
        eng = Engine(U, N, k, e, B, **hp)
        eng.set_urm(urm)
        for n, tid in NAME2ID.items():
            eng.set_tensor(tid, p0[n])
        losses[run] = [eng.train_epoch(p, d_steps, g_steps) for p in perms]
        errs[run] = {n: _err(eng.get_tensor(tid), o.p[n]) for n, tid in NAME2ID.items()}
        eng.close()
    for run in errs:
        for (dl, gl), (dl_ref, gl_ref) in zip(losses[run], refs):
            np.testing.assert_allclose(dl, dl_ref, rtol=ltol, atol=1e-7, err_msg=run + " " + what)
            np.testing.assert_allclose(gl, gl_ref, rtol=ltol, atol=1e-7, err_msg=run + " " + what)
        for n in NAME2ID:
            assert errs[run][n] <= max(2e-4, 2.0 * fp32[n]), (run, n, errs[run][n], fp32[n], what)
    if all(v <= 2e-4 for v in fp32.values()):
        for n in NAME2ID:
            assert errs[mode][n] <= 2.0 * max(errs["dense"][n], fp32[n]) + 1e-6, (n, errs[mode][n], errs["dense"][n], fp32[n], what)
    assert _paths(capfd) == [_expect(mode), (0, 0)]


# -- 3: gradients of one step, row by row ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sparse_g", "sparse_gd"])
@pytest.mark.parametrize("e", [37, 1030])
def test_one_step_gradients_row_by_row(mode, e, monkeypatch, capfd):
    """From zero moments one step leaves SLOT_ADAM_M = (1 - beta1) g: gWe, gbe, gWd, gbd after one D step and gU, gV after the G step
    that follows, row by row against GANMFOracle.d_grads / g_grads, each row normalised by its own fp64 |terms| bound (not by the
    tensor's largest element: one wrong item row of gWe -- an empty CSC column, the column beside the bias row, the float4 tail --
    must fail).  Three calls: ganmf_train_step on an explicit id list of 5 rows (< CSC_BIAS_PARTS), on 40 rows, and an epoch over a
    partial permutation (pos = -1 for every row left out) of one ragged minibatch; every call holds a row of more than 2 000 ratings."""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    U, N, k, B = 60, 2300, 9, 40
    rng = np.random.RandomState(e)
    urm = _rated_urm(rng, U, N, 0.02, "ratings", long_row=True)
    assert np.any(np.diff(urm.tocsc().indptr) == 0) and urm[:, N - 1].nnz > 0 and urm[0].nnz > 2000
    hp = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-3, g_reg=0.0, m=5.0, recon_coefficient=0.3)
    o0 = GANMFOracle(U, N, k, e, dtype=np.float64, seed=9, **hp)
    o0.set_params(be=rng.randn(e) * 0.01, bd=rng.randn(N) * 0.01)
    p0 = o0.get_params()
    one_minus_b1 = np.float64(np.float32(1.0) - np.float32(0.9))
    calls = [(how, np.concatenate([[0], rng.choice(np.arange(1, U), n - 1, replace=False)])[rng.permutation(n)])
             for how, n in (("step", 5), ("step", 40), ("epoch", 23))]      # (row 0: the long row)
    _set_mode(monkeypatch, mode)
    capfd.readouterr()
    for how, uids in calls:
        o = GANMFOracle(U, N, k, e, dtype=np.float64, **hp)
        o.set_params(**p0)
        X = urm[uids].toarray().astype(np.float64)
        _, gd = o.d_grads(uids, X)
        bd = _abs_d_bounds(o, uids, X)
        o.d_step(uids, X)
        _, gg = o.g_grads(uids, X)
        bg = _abs_g_bounds(o, uids, X)
        eng = Engine(U, N, k, e, B, **hp)
        eng.set_urm(urm)
        for n, tid in NAME2ID.items():
            eng.set_tensor(tid, p0[n])
        if how == "step":
            eng.train_step(0, uids)
            eng.train_step(1, uids)
        else:
            eng.train_epoch(uids, 1, 1)
        for n, ref, bound in [(n, gd[n], bd[n]) for n in o.D_NAMES] + [(n, gg[n], bg[n]) for n in o.G_NAMES]:
            got = eng.get_tensor(NAME2ID[n], slot=L.SLOT_ADAM_M).astype(np.float64) / one_minus_b1
            _rowwise(got, ref, bound, (mode, e, how, len(uids), n))
        eng.close()
    assert _paths(capfd) == [_expect(mode)] * len(calls)


# -- 4: schedule forms under the sparse path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sparse_g", "sparse_gd"])
def test_per_pass_forms_bit_identical_on_the_sparse_path(mode, monkeypatch, capfd):
    """test_gpu_multi_launch.py::test_per_pass_forms_are_bit_identical with the sparse real path forced: d_steps = 2, g_steps = 3, the
    second epoch a call that leaves a third of the rows out; every GANMF_TUNE combination of pass_stage / lazy_rows / g_rows_staged
    gives the per-step forms' losses, parameters and both moments bit for bit."""
    U, N, k, e, B = 700, 1100, 20, 66, 32
    hp = dict(d_lr=1e-4, g_lr=2e-4, d_reg=1e-4, g_reg=0.0, m=10.0, recon_coefficient=0.05)
    _set_mode(monkeypatch, mode)
    capfd.readouterr()
    ref, ref_l = _run_staged(monkeypatch, "pass_stage=0,lazy_rows=0", "ganmf", U, N, k, e, B, hp, 2, 2, 3)
    tunes = ("pass_stage=1,lazy_rows=0", "pass_stage=0,lazy_rows=1", "pass_stage=1,lazy_rows=1", "pass_stage=1,lazy_rows=1,g_rows_staged=0",
             "pass_stage=1,lazy_rows=1,g_rows_staged=2")
    for tune in tunes:
        got, got_l = _run_staged(monkeypatch, tune, "ganmf", U, N, k, e, B, hp, 2, 2, 3)
        for (dl, gl), (dr, gr) in zip(got_l, ref_l):
            np.testing.assert_array_equal(dl, dr, err_msg="D losses, %s, %s" % (mode, tune))
            np.testing.assert_array_equal(gl, gr, err_msg="G losses, %s, %s" % (mode, tune))
        assert set(ref) == set(got)
        for n in ref:
            np.testing.assert_array_equal(got[n], ref[n], err_msg="%s, %s, %s" % (n, mode, tune))
    assert _paths(capfd) == [_expect(mode)] * (1 + len(tunes))


# -- 5: loopback data-parallel step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,world,U", [("forced", 2, 33), ("forced", 3, 49), ("straddle", 2, 33)])
def test_sharded_epoch_on_the_sparse_path(case, world, U, monkeypatch, capfd):
    """test_gpu_dist_local.py::test_ganmf_sharded_epoch_equals_union_batch on the sparse real path: ragged shards of B = 8 that leave
    some rank with no rows in the last step (nb == 0: the sparse kernels launch on an empty batch).  "forced": GANMF_SPARSE = 1,
    GANMF_SPARSE_D = 1 on every rank.  "straddle": no override; rank 0's shard is 0.2 % dense, rank 1's 2 %, so the planner puts
    rank 0 on the sparse generator path and rank 1 on the dense one inside the same data-parallel step.  Union-batch oracle;
    replicated tensors bitwise equal on every rank."""
    from ganmf_amd.engine import Engine
    N, k, e, B = (61, 5, 9, 8) if case == "forced" else (2000, 5, 9, 8)
    rng = np.random.RandomState(world + 40)
    bounds = shard_bounds(U, world)
    if case == "forced":
        urm = _rated_urm(rng, U, N, 0.15, "ratings")
        _set_mode(monkeypatch, "sparse_gd")
        expect = [(1, 1)] * world
    else:
        dens = np.zeros(U)
        dens[bounds[0][0]:bounds[0][1]], dens[bounds[1][0]:bounds[1][1]] = 0.002, 0.02
        m = rng.rand(U, N) < dens[:, None]
        m[:, N - 1] |= rng.rand(U) < 0.1
        vals = np.zeros((U, N), np.float32)
        vals[m] = _values(rng, int(m.sum()), "plays")
        urm = sps.csr_matrix(vals)
        for (lo, hi), below in zip(bounds, (True, False)):
            assert (urm[lo:hi].nnz / ((hi - lo) * N) < 0.005) == below
        _set_mode(monkeypatch, None)
        expect = [(1, 0), (0, 0)]
    steps_rows = [[min(B, max(0, (hi - lo) - i * B)) for (lo, hi) in bounds] for i in range(-(-max(b - a for a, b in bounds) // B))]
    assert 0 in steps_rows[-1]      # some rank has no rows in the last step
    hp = dict(d_lr=1e-3, g_lr=2e-3, d_reg=1e-3, g_reg=1e-4, m=10.0, recon_coefficient=0.2)
    o = GANMFOracle(U, N, k, e, dtype=np.float64, seed=3, **hp)
    o.set_params(be=rng.randn(e) * 0.01, bd=rng.randn(N) * 0.01)
    p0 = o.get_params()
    perms = [rng.permutation(b - a) for a, b in bounds]

    def make_engine(r):
        lo, hi = bounds[r]
        eng = Engine(hi - lo, N, k, e, B, world_size=world, rank=r, row_offset=lo, **hp)
        eng.set_urm(urm[lo:hi])
        for n, tid in (("We", 0), ("be", 1), ("Wd", 2), ("bd", 3), ("V", 101)):
            eng.set_tensor(tid, p0[n])
        eng.set_tensor(100, p0["U"][lo:hi])
        return eng

    capfd.readouterr()
    engines, out, steps = _run_ranks(world, make_engine, bounds, perms, B, group=300 + world + (10 if case == "straddle" else 0))
    assert _paths(capfd) == expect
    unions = [np.concatenate([bounds[r][0] + perms[r][i * B:(i + 1) * B] for r in range(world)]) for i in range(steps)]
    dl_ref = [o.d_step(u, urm[u].toarray()) for u in unions]
    gl_ref = [o.g_step(u, urm[u].toarray()) for u in unions]
    for r in range(world):
        np.testing.assert_allclose(out[r][0], dl_ref, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(out[r][1], gl_ref, rtol=1e-4, atol=1e-7)
    for n, tid in (("We", 0), ("be", 1), ("Wd", 2), ("bd", 3), ("V", 101)):
        t0 = engines[0].get_tensor(tid)
        assert _err(t0, o.p[n]) <= 1e-4, n
        for r in range(1, world):
            assert np.array_equal(engines[r].get_tensor(tid), t0), (n, r)
    for r, (lo, hi) in enumerate(bounds):
        assert _err(engines[r].get_tensor(100), o.p["U"][lo:hi]) <= 1e-4, r
    for eng in engines:
        eng.close()


# -- 6: weighted values on the dense paths --------------------------------------------------------------------------------------
def test_ganmf_dense_path_rated_urm(monkeypatch, capfd):
    """test_gpu_parity.py::test_epochs_match_oracle_ragged with ratings 1-5 in place of ones, on the planner's dense path."""
    from ganmf_amd.engine import Engine
    U, N, k, e, B = 101, 160, 12, 20, 16
    rng = np.random.RandomState(8)
    urm = _rated_urm(rng, U, N, 0.07, "ratings")
    hp = dict(d_lr=1e-3, g_lr=2e-3, d_reg=1e-4, g_reg=1e-5, m=5.0, recon_coefficient=0.3)
    o = GANMFOracle(U, N, k, e, dtype=np.float64, seed=2, **hp)
    _set_mode(monkeypatch, None)
    capfd.readouterr()
    eng = Engine(U, N, k, e, B, **hp)
    eng.set_urm(urm)
    for n, tid in NAME2ID.items():
        eng.set_tensor(tid, o.p[n])
    assert _paths(capfd) == [(0, 0)]
    for _ in range(3):
        perm = rng.permutation(U)
        dl_ref, gl_ref = o.train_epoch(urm, perm, B, 2, 2)
        dl, gl = eng.train_epoch(perm, 2, 2)
        np.testing.assert_allclose(dl, dl_ref, rtol=5e-5, atol=1e-7)
        np.testing.assert_allclose(gl, gl_ref, rtol=5e-5, atol=1e-7)
    for n, tid in NAME2ID.items():
        assert _err(eng.get_tensor(tid), o.p[n]) <= 1e-4, n
    assert _err(eng.scores(np.arange(U)), o.scores(np.arange(U))) <= 1e-4
    eng.close()


@pytest.mark.parametrize("mfma", [None, "f16"])
def test_disganmf_rated_urm(mfma):
    """DisGANMF, 2 tanh layers, the float(uid) column, ratings 1-5: three epochs against the oracle at
    test_gpu_disganmf.py::test_disganmf_epochs_ragged_tanh2's tolerances; fp16 MFMA inputs (ratings are exact in fp16) three steps at
    test_gpu_mfma_modes.py::test_disganmf_f16_hidden_layers' tolerances (losses 5e-3, first moments 2e-2 of their scale)."""
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    layers, act = 2, "tanh"
    rng = np.random.RandomState(13)
    if mfma is None:
        U, N, k, e, B = 101, 160, 12, 20, 16
        hp = dict(d_lr=1e-3, g_lr=2e-3, d_reg=1e-4, g_reg=0.0, recon_coefficient=0.3)
        urm = _rated_urm(rng, U, N, 0.07, "ratings")
    else:
        U, N, k, e, B = 300, 500, 16, 96, 64
        hp = dict(d_lr=1e-3, g_lr=1e-3, d_reg=1e-4, g_reg=0.0, recon_coefficient=0.3)
        urm = _rated_urm(rng, U, N, 0.05, "ratings")
    o = DisGANMFOracle(U, N, k, d_layers=layers, d_nodes=e, d_hidden_act=act, dtype=np.float64, seed=4, **hp)
    if mfma is None:
        o.p["W0"][0, :] *= 1.0 / U
    eng = Engine(U, N, k, e, B, model=L.MODEL_DISGANMF, d_layers=layers, d_act=act, m=0.0, mfma=mfma, **hp)
    eng.set_urm(urm)
    ids = {"W0": 0, "b0": 1, "W1": 2, "b1": 3, "Wo": 4, "bo": 5, "U": 100, "V": 101}
    for n, tid in ids.items():
        eng.set_tensor(tid, o.p[n])
    if mfma is None:
        for _ in range(3):
            perm = rng.permutation(U)
            dl_ref, gl_ref = o.train_epoch(urm, perm, B, 1, 1)
            dl, gl = eng.train_epoch(perm, 1, 1)
            np.testing.assert_allclose(dl, dl_ref, rtol=1e-4, atol=1e-7)
            np.testing.assert_allclose(gl, gl_ref, rtol=1e-4, atol=1e-7)
        for n, tid in ids.items():
            assert _err(eng.get_tensor(tid), o.p[n]) <= 2e-4, n
    else:
        perm = rng.permutation(U)
        for t in range(3):
            uids = perm[t * B:(t + 1) * B]
            X = urm[uids].toarray()
            ld_ref, ld = o.d_step(uids, X), eng.train_step(0, uids)
            lg_ref, lg = o.g_step(uids, X), eng.train_step(1, uids)
            assert abs(ld - ld_ref) <= 5e-3 * abs(ld_ref) + 1e-5, (t, ld, ld_ref)
            assert abs(lg - lg_ref) <= 5e-3 * abs(lg_ref) + 1e-5, (t, lg, lg_ref)
        for n, tid in ids.items():
            m_ref = (o.opt_d.slots[n] if n in o.opt_d.slots else o.opt_g.slots[n])[0]
            assert _err(eng.get_tensor(tid, slot=L.SLOT_ADAM_M), m_ref) <= 2e-2, n
    eng.close()
