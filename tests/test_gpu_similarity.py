"""Prediction cosine-similarity study on the device (ganmf_score_similarity, ganmf_amd/csrc/gram_stats.hpp) through the C ABI, the
Engine and the classes: the computation under the reference's collapse study (AblationStudy.py:88-92,113-117).

Bound against the fp64 oracle (tests/helpers_similarity.py), for the matrix entry-wise, the pooled block means, the mean and the
std: the device may deviate from fp64 by at most 4 x the deviation of the float32 restatement of the reference's own sequence on
the same inputs (the project's rule for fp32-accurate paths that sum in another order than numpy, tests/test_gpu_trajectory.py),
with the floor sqrt(W) * 2^-23: the expected rounding of a W-term float32 dot product of unit vectors.  Every case prints
`ratio = deviation / allowed`.

Shapes: n in {1, 63, 64, 65, 129, 200, 257} -- the Gram kernel walks 128 x 128 tiles, so 1..65 is one diagonal tile with ragged
edges, 129 and 200 a diagonal plus an off-diagonal tile (weight 2, mirror store), 257 three tile rows of the triangular map;
widths 70 and 257 (K tails, pad columns), k in {8, 40}, user and item mode; ids are a shuffled subset with one id repeated."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from tests.helpers_similarity import oracle64, pooled_means, restatement32, restatement32_stats

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 129, 200, 257]
DOMAIN = 300          # rows of the scored side


def _engine(rows, cols, item_mode):
    """an engine whose scored side holds `rows` and whose other factor holds `cols` (item mode: the roles of U and V swap)"""
    from ganmf_amd.engine import Engine
    U, V = (cols, rows) if item_mode else (rows, cols)
    eng = Engine(U.shape[0], V.shape[0], U.shape[1], 16, 32)
    eng.set_tensor(100, U)
    eng.set_tensor(101, V)
    return eng


def _ids(rng, n, domain=DOMAIN):
    """n ids: a shuffled subset with one id repeated (n >= 2)"""
    if n == 1:
        return rng.choice(domain, size=1).astype(np.int32)
    ids = rng.choice(domain, size=n - 1, replace=False)
    ids = np.concatenate([ids, ids[:1]])
    return ids[rng.permutation(n)].astype(np.int32)


@pytest.fixture(scope="module")
def cases():
    """(W, k, item_mode) -> (engine, rows, cols): built once, shared, never modified"""
    held = {}

    def get(W, k, item_mode):
        key = (W, k, item_mode)
        if key not in held:
            rng = np.random.RandomState(1000 * W + 10 * k + int(item_mode))
            rows = rng.randn(DOMAIN, k).astype(np.float32)
            cols = rng.randn(W, k).astype(np.float32)
            held[key] = (_engine(rows, cols, item_mode), rows, cols)
        return held[key]
    yield get
    for eng, _, _ in held.values():
        eng.close()


def _allowed(ref_dev, W):
    return max(4.0 * ref_dev, np.sqrt(W) * 2.0 ** -23)


def _check_against_oracle(label, got, rows, cols, pool=None):
    """got: score_similarity's dict for the factor rows `rows` (already gathered); every deviation against the 4 x rule"""
    W = cols.shape[0]
    o = oracle64(rows, cols)
    c32 = restatement32(rows, cols)
    m32, s32 = restatement32_stats(c32)
    worst = 0.0
    for name, dev, ref in (("mean", abs(got["mean"] - o["mean"]), abs(m32 - o["mean"])),
                           ("std", abs(got["std"] - o["std"]), abs(s32 - o["std"]))):
        ratio = dev / _allowed(ref, W)
        print("%s %s: deviation %.3e, restatement %.3e, ratio %.3f" % (label, name, dev, ref, ratio))
        worst = max(worst, ratio)
    if "matrix" in got:
        dev = np.abs(got["matrix"].astype(np.float64) - o["matrix"]).max()
        ref = np.abs(c32.astype(np.float64) - o["matrix"]).max()
        ratio = dev / _allowed(ref, W)
        print("%s matrix: deviation %.3e, restatement %.3e, ratio %.3f" % (label, dev, ref, ratio))
        worst = max(worst, ratio)
    if pool is not None:
        want = pooled_means(o["matrix"], pool)
        dev = np.abs(got["pooled"].astype(np.float64) - want).max()
        ref = np.abs(pooled_means(c32, pool) - want).max()
        ratio = dev / _allowed(ref, W)
        print("%s pooled: deviation %.3e, restatement %.3e, ratio %.3f" % (label, dev, ref, ratio))
        worst = max(worst, ratio)
    assert got["zero_rows"] == o["zero_rows"] and got["n"] == rows.shape[0]
    assert worst <= 1.0, (label, worst)
    return o


@pytest.mark.parametrize("item_mode", [False, True])
@pytest.mark.parametrize("k", [8, 40])
@pytest.mark.parametrize("W", [70, 257])
@pytest.mark.parametrize("n", NS)
def test_bound_against_fp64(cases, n, W, k, item_mode):
    eng, rows, cols = cases(W, k, item_mode)
    ids = _ids(np.random.RandomState(n + W + k), n)
    pool = min(n, 5)
    got = eng.score_similarity(ids, transposed=item_mode, pool=pool, return_matrix=True)
    label = "n=%d W=%d k=%d %s" % (n, W, k, "item" if item_mode else "user")
    _check_against_oracle(label, got, rows[ids], cols, pool=pool)
    c = got["matrix"]
    assert np.array_equal(c, c.T)                     # the mirror store
    if n > 1:                                        # the repeated id: c = 1 off the diagonal
        a, b = [np.flatnonzero(ids == v) for v in ids if (ids == v).sum() == 2][0]
        assert abs(c[a, b] - 1.0) <= _allowed(0.0, W) and c[a, b] == c[b, a]
    stats = eng.score_similarity(ids, transposed=item_mode)
    assert (stats["sum_d"], stats["sum_d2"]) == (got["sum_d"], got["sum_d2"]) and "matrix" not in stats and "pooled" not in stats


def _exact_factors(rng, k, W):
    """scored side: rows of exactly 4 or 16 entries of +-1; other side: one-hot rows e_0 .. e_(k-1), then zero rows -- every score
    row then has exactly 4 or 16 entries of +-1 and zeros elsewhere: norms 2 or 4, every s^, c and d exactly representable"""
    rows = np.zeros((DOMAIN, k), dtype=np.float32)
    for r in range(DOMAIN):
        nz = 16 if (k >= 16 and r % 3 == 0) else 4
        rows[r, rng.choice(k, size=nz, replace=False)] = rng.choice([-1.0, 1.0], size=nz)
    cols = np.zeros((W, k), dtype=np.float32)
    cols[np.arange(k), np.arange(k)] = 1.0
    return rows, cols


@pytest.fixture(scope="module")
def exact_cases():
    held = {}

    def get(item_mode):
        if item_mode not in held:
            rows, cols = _exact_factors(np.random.RandomState(7 + int(item_mode)), 40, 70)
            held[item_mode] = (_engine(rows, cols, item_mode), rows, cols)
        return held[item_mode]
    yield get
    for eng, _, _ in held.values():
        eng.close()


@pytest.mark.parametrize("item_mode", [False, True])
@pytest.mark.parametrize("n", NS)
def test_exact_case_is_bitwise(exact_cases, n, item_mode):
    eng, rows, cols = exact_cases(item_mode)
    ids = _ids(np.random.RandomState(3 * n), n)
    o = oracle64(rows[ids], cols)
    want = o["matrix"].astype(np.float32)
    assert np.array_equal(want.astype(np.float64), o["matrix"])      # the construction: every c is a float32 number
    got = eng.score_similarity(ids, transposed=item_mode, return_matrix=True)
    assert np.array_equal(got["matrix"], want)
    assert got["sum_d"] == o["sum_d"] and got["sum_d2"] == o["sum_d2"]
    stats = eng.score_similarity(ids, transposed=item_mode)
    assert stats["sum_d"] == o["sum_d"] and stats["sum_d2"] == o["sum_d2"]
    assert stats["mean"] == o["mean"] and stats["std"] == o["std"]


@pytest.mark.parametrize("item_mode", [False, True])
def test_zero_rows(item_mode):
    rng = np.random.RandomState(11)
    rows = rng.randn(DOMAIN, 8).astype(np.float32)
    cols = rng.randn(70, 8).astype(np.float32)
    rows[[17, 203]] = 0.0
    eng = _engine(rows, cols, item_mode)
    try:
        ids = rng.permutation(DOMAIN)[:129].astype(np.int32)
        ids[5], ids[100] = 17, 203
        got = eng.score_similarity(ids, transposed=item_mode, return_matrix=True)
        assert got["zero_rows"] == 2
        for z in (5, 100):
            assert np.all(got["matrix"][z] == 0) and np.all(got["matrix"][:, z] == 0)
        o = _check_against_oracle("zero rows", got, rows[ids], cols)
        assert o["matrix"][5, 5] == 0 and o["zero_rows"] == 2
    finally:
        eng.close()


def test_pooling(cases):
    eng, rows, cols = cases(257, 40, False)
    ids = _ids(np.random.RandomState(5), 200)
    full = eng.score_similarity(ids, return_matrix=True)
    one = eng.score_similarity(ids, pool=1)
    assert one["pooled"].shape == (1, 1) and abs(float(one["pooled"][0, 0]) - one["mean"]) <= 2.0 ** -23
    alln = eng.score_similarity(ids, pool=200)
    assert np.array_equal(alln["pooled"], full["matrix"])
    seven = eng.score_similarity(ids, pool=7, return_matrix=True)
    _check_against_oracle("pool=7 n=200", seven, rows[ids], cols, pool=7)
    # the block means are those of the device's own matrix (float64 sums, one rounding)
    assert np.abs(seven["pooled"].astype(np.float64) - pooled_means(seven["matrix"], 7)).max() <= 2.0 ** -24


def test_determinism(cases):
    eng, rows, cols = cases(257, 40, False)
    other = _engine(rows, cols, False)
    try:
        ids = _ids(np.random.RandomState(9), 257)
        runs = [e.score_similarity(ids, pool=7, return_matrix=True) for e in (eng, eng, other)]
        for r in runs[1:]:
            assert r["matrix"].tobytes() == runs[0]["matrix"].tobytes() and r["pooled"].tobytes() == runs[0]["pooled"].tobytes()
            assert (r["sum_d"], r["sum_d2"], r["zero_rows"]) == (runs[0]["sum_d"], runs[0]["sum_d2"], runs[0]["zero_rows"])
    finally:
        other.close()


def test_second_arithmetic_candidate(monkeypatch):
    """GANMF_TUNE=gram=0: the plain fp32 MFMA instead of the default exact three-way bf16 split, held to the same bound"""
    monkeypatch.setenv("GANMF_TUNE", "gram=0")
    rng = np.random.RandomState(21)
    rows = rng.randn(DOMAIN, 40).astype(np.float32)
    cols = rng.randn(257, 40).astype(np.float32)
    eng = _engine(rows, cols, False)
    try:
        for n in (65, 257):
            ids = _ids(rng, n)
            got = eng.score_similarity(ids, pool=min(n, 7), return_matrix=True)
            _check_against_oracle("fp32 MFMA n=%d" % n, got, rows[ids], cols, pool=min(n, 7))
        erows, ecols = _exact_factors(rng, 40, 70)
        exact = _engine(erows, ecols, False)
        try:
            ids = _ids(rng, 200)
            o = oracle64(erows[ids], ecols)
            got = exact.score_similarity(ids, return_matrix=True)
            assert np.array_equal(got["matrix"], o["matrix"].astype(np.float32))
            assert got["sum_d"] == o["sum_d"] and got["sum_d2"] == o["sum_d2"]
        finally:
            exact.close()
    finally:
        eng.close()


def test_no_side_effects(cases):
    from ganmf_amd import _lib as L
    eng, rows, cols = cases(70, 8, False)
    ids = _ids(np.random.RandomState(13), 65)

    def state():
        out = [eng.scores(ids), eng.adam_powers()]
        for tid in (100, 101, 0, 1, 2, 3):
            for slot in (L.SLOT_PARAM, L.SLOT_ADAM_M, L.SLOT_ADAM_V):
                out.append(eng.get_tensor(tid, slot))
        return out
    before = state()
    plain = eng.score_similarity(ids, pool=5, return_matrix=True)
    for a, b in zip(before, state()):
        assert a.tobytes() == b.tobytes()
    # with a score filter set (what score_contract="mf" sets): the similarity is the unfiltered one, the filter stays
    seen = sps.csr_matrix((np.ones(3, np.float32), ([0, 1, 2], [0, 1, 2])), shape=(DOMAIN, 70))      # most rows are cold
    eng.set_seen(seen)
    keep = np.array([3, 4, 9], dtype=np.int32)
    eng.set_score_filter(keep, mask_cold=True)
    try:
        filtered = eng.score_similarity(ids, pool=5, return_matrix=True)
        assert filtered["matrix"].tobytes() == plain["matrix"].tobytes() and filtered["pooled"].tobytes() == plain["pooled"].tobytes()
        assert (filtered["sum_d"], filtered["sum_d2"]) == (plain["sum_d"], plain["sum_d2"])
        s = eng.scores(np.arange(4, dtype=np.int32))
        others = np.setdiff1d(np.arange(70), keep)
        assert np.all(np.isneginf(s[:, others])) and np.all(np.isfinite(s[:3][:, keep])) and np.all(np.isneginf(s[3]))
    finally:
        eng.set_score_filter(None, mask_cold=False)
    assert eng.scores(ids).tobytes() == before[0].tobytes()


def test_errors_leave_the_handle_usable(cases):
    from ganmf_amd import _lib as L
    eng, rows, cols = cases(70, 8, False)
    lib = L.load_library()
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    good = np.arange(10, dtype=np.int32)
    sums = np.zeros(4)
    pooled = np.zeros((16, 16), dtype=np.float32)

    def call(ids, n, pool, pooled_buf):
        return lib.ganmf_score_similarity(eng.h, ids.ctypes.data_as(ip), n, 0, pool, sums.ctypes.data_as(dp),
                                          pooled_buf.ctypes.data_as(fp) if pooled_buf is not None else None, None)
    bad = good.copy()
    bad[4] = DOMAIN
    neg = good.copy()
    neg[0] = -1
    for what, rc in (("id out of range", call(bad, 10, 0, None)), ("negative id", call(neg, 10, 0, None)),
                     ("n = 0", call(good, 0, 0, None)), ("pool = 0", call(good, 10, 0, pooled)),
                     ("pool > n", call(good, 10, 11, pooled)), ("null ids", lib.ganmf_score_similarity(
                         eng.h, None, 10, 0, 0, sums.ctypes.data_as(dp), None, None)),
                     ("null sums", lib.ganmf_score_similarity(eng.h, good.ctypes.data_as(ip), 10, 0, 0, None, None, None))):
        assert rc == -1, what
        assert lib.ganmf_last_error(), what
    with pytest.raises(L.GanmfError):
        eng.score_similarity(good, pool=0)
    with pytest.raises(L.GanmfError):
        eng.score_similarity(good, pool=11)
    assert call(good, 10, 10, pooled) == 0
    got = eng.score_similarity(good, pool=2, return_matrix=True)
    _check_against_oracle("after errors", got, rows[good], cols, pool=2)


def test_profile_class(cases):
    eng, rows, cols = cases(70, 8, False)
    eng.profile(True)
    try:
        eng.score_similarity(np.arange(65, dtype=np.int32), pool=3)
        names = {e["name"]: e for e in eng.profile_read()}
    finally:
        eng.profile(False)
    gram = [e for name, e in names.items() if name.startswith("gram_similarity")]
    assert len(gram) == 1 and gram[0]["launches"] == 1 and gram[0]["flops"] > 0


@pytest.mark.parametrize("cls,mode,contract", [("GANMF", "user", None), ("GANMF", "item", "mf"), ("DisGANMF", "user", None)])
def test_through_the_classes(cls, mode, contract):
    from ganmf_amd.DisGANMF import DisGANMF
    from ganmf_amd.GANMF import GANMF
    rng = np.random.RandomState(31)
    urm = sps.csr_matrix((rng.rand(140, 90) < 0.1).astype(np.float32))
    model = {"GANMF": GANMF, "DisGANMF": DisGANMF}[cls](urm, mode=mode, is_experiment=True, score_contract=contract)
    with pytest.raises(RuntimeError):
        model.prediction_similarity()            # no device state yet: raises like every other scoring call
    if cls == "GANMF":
        model._build(8, 16, 32)
    else:
        model._build_dis(8, 1, 16, "linear", 32)
    try:
        fu, fv = model.engine.shape(100), model.engine.shape(101)
        model.engine.set_tensor(100, rng.randn(*fu).astype(np.float32))
        model.engine.set_tensor(101, rng.randn(*fv).astype(np.float32))
        rows, cols = model.USER_factors, model.ITEM_factors      # evaluation orientation
        assert rows.shape[0] == 140 and cols.shape[0] == 90
        got = model.prediction_similarity(pool=9, return_matrix=True)      # None: every user, as AblationStudy.py:88 passes
        assert got["n"] == 140
        _check_against_oracle("%s %s all users" % (cls, mode), got, rows, cols, pool=9)
        some = np.array([5, 139, 0, 77, 5])
        got = model.prediction_similarity(some)
        assert set(got) >= {"mean", "std", "n", "zero_rows"} and "matrix" not in got and "pooled" not in got
        _check_against_oracle("%s %s subset" % (cls, mode), got, rows[some], cols)
    finally:
        model.engine.close()


def _factor_space_stats(rows, cols):
    """mean and population std of the full cosine matrix in float64 without forming it: with M = cols^T cols and the row norms
    ||s_i||^2 = r_i M r_i^T, sum(c) = v M v^T for v = sum_i r_i / ||s_i||, and sum(c^2) = tr(P M P M) for
    P = sum_i r_i^T r_i / ||s_i||^2 (the same numbers as oracle64's up to float64 rounding; checked below at a small shape)"""
    r, c = rows.astype(np.float64), cols.astype(np.float64)
    M = c.T @ c
    norm2 = np.einsum("ik,kl,il->i", r, M, r)
    rn = r / np.sqrt(norm2)[:, None]
    v = rn.sum(axis=0)
    P = rn.T @ rn
    n = r.shape[0]
    mean = float(v @ M @ v) / (float(n) * n)
    mean_sq = float(np.trace(P @ M @ P @ M)) / (float(n) * n)
    return mean, float(np.sqrt(max(mean_sq - mean * mean, 0.0)))


@pytest.fixture(scope="module")
def real_shape():
    rng = np.random.RandomState(2024)
    rows = (rng.randn(6040, 250) / np.sqrt(250)).astype(np.float32)
    rows += 0.3 * rows[:1]                       # a partly collapsed generator: the mean is well away from 0
    cols = rng.randn(3706, 250).astype(np.float32)
    eng = _engine(rows, cols, False)
    yield eng, rows, cols
    eng.close()


def test_real_shape_sampled_rows(real_shape):
    """ML-1M shape (6040 x 3706 x 250), statistics only, the oracle evaluated on 257 sampled rows (the trajectory test's sampling)"""
    eng, rows, cols = real_shape
    probe = np.random.RandomState(1).permutation(6040)[:257].astype(np.int32)
    got = eng.score_similarity(probe)
    _check_against_oracle("6040x3706x250, 257 sampled rows", got, rows[probe], cols)


def test_real_shape_all_rows(real_shape):
    """All 6040 rows, statistics only: 48 tile rows of the triangular map, 1176 tiles.  The 6040^2 fp64 matrix is not formed: its mean and
    std follow from k x k matrices in float64 (_factor_space_stats).  Bound: every entry's error e is that of a W-term float32 dot
    product of unit vectors, 4 * sqrt(W) * 2^-23 by the rule above; the mean moves by at most max|e|, and so does the population std
    (it is 1-Lipschitz in the RMS of a perturbation of the entries)."""
    eng, rows, cols = real_shape
    small = np.arange(0, 6040, 47)
    o = oracle64(rows[small], cols)
    m, s = _factor_space_stats(rows[small], cols)
    assert abs(m - o["mean"]) <= 1e-12 and abs(s - o["std"]) <= 1e-10
    mean, std = _factor_space_stats(rows, cols)
    got = eng.score_similarity(np.arange(6040, dtype=np.int32))
    allowed = 4.0 * np.sqrt(3706) * 2.0 ** -23
    print("6040 rows: mean %.9f (fp64 %.9f), std %.9f (fp64 %.9f), ratios %.3f %.3f"
          % (got["mean"], mean, got["std"], std, abs(got["mean"] - mean) / allowed, abs(got["std"] - std) / allowed))
    assert got["n"] == 6040 and got["zero_rows"] == 0
    assert abs(got["mean"] - mean) <= allowed and abs(got["std"] - std) <= allowed
