"""The split-bf16 K loops at the edges of their address code (gemm_bf16k.hpp, gemm_bf16w.hpp, gemm_bf16s.hpp): the operand addresses of
a K-tile are a per-lane pointer stepped once per tile, the zero-page selects of a partial last K-tile sit behind a scalar branch, and
the LDS addresses of planes, pieces and buffers are formed once in front of the loop.  What can go wrong there is a tile that takes the
wrong side of that branch, a slice shorter than the prefetch depth, a lane outside the operand that steps off its zero-page line, or
a plane buffer addressed with the other buffer's base -- so: K on and around the K-tile (64; 128 for the 64 x 32 kernel, 32 for the
4-wave one), forced splits that give slices of 1, 2 and 3 K-tiles and slices that end inside a K-tile, ragged rows and columns, every
layout, gathered A rows with repeated ids, and the fused-Adam epilogue behind the 4-wave TN loop.

Reference: the fp64 product in numpy; bound: the one tests/test_gpu_gemm.py uses for these kernels, 4e-7 * sqrt(K) * sum |a||b|.
Every product is run twice and must give the same bits."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = {"NT": (False, False), "NN": (False, True), "TN": (True, True)}
KS = [1, 63, 64, 65, 127, 129, 191, 250, 993]
MS = [1, 63, 65, 128]
NS = [33, 64, 96]
MN = [(m, n) for m in MS for n in NS]


@functools.lru_cache(maxsize=None)
def _case(M, N, K, akm, bkm, rows=0):
    """operands, fp64 product and sum |a||b| -- built once per shape and shared (never written to) by the tests that use it;
    rows > 0: A is a table of `rows` rows and the product's row r is table row ids[r] (repeated ids)"""
    rng = np.random.RandomState(M * 131 + N * 17 + K * 3 + 2 * akm + bkm + 1000 * rows)
    ids = None
    if rows:
        ids = rng.randint(0, rows, M).astype(np.int32)
        ids[-1] = ids[0]      # at least one repeated id, whatever the draw
        A = rng.standard_normal((rows, K)).astype(np.float32)
        Am = A[ids]
    else:
        A = rng.standard_normal((K, M) if akm else (M, K)).astype(np.float32)
        Am = A.T if akm else A
    B = rng.standard_normal((K, N) if bkm else (N, K)).astype(np.float32)
    Bm = B if bkm else B.T
    ref = Am.astype(np.float64) @ Bm.astype(np.float64)
    bound = np.abs(Am).astype(np.float64) @ np.abs(Bm).astype(np.float64)
    for a in (A, B, ref, bound):
        a.setflags(write=False)
    return A, B, ref, bound, ids


def _check(out, ref, bound, K, what):
    err = np.abs(out - ref)
    worst = float((err / (bound + 1e-30)).max())
    print("%s: max err / sum|a||b| = %.3e (bound %.3e)" % (what, worst, 4e-7 * np.sqrt(K)))
    assert np.all(err <= 4e-7 * bound * np.sqrt(K) + 1e-30), (what, worst)


def _x3kg_env(monkeypatch):
    # the 16-wave split-bf16 kernel through the stand-alone entry, as tests/test_gpu_gemm.py selects it
    monkeypatch.setenv("GANMF_MFMA", "f32")
    monkeypatch.setenv("GANMF_TUNE", "kg=4,ring=3")
    monkeypatch.setenv("GANMF_X3KG", "3")


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_kloop_16wave_k_edges(layout, nsplit, monkeypatch):
    """gemm_bf16k_mfma: every K of the list in every layout and forced split; the (M, N) pairs rotate through the K's so that every
    pair meets every layout (nine K's x three splits against twelve pairs)"""
    from ganmf_amd.engine import gemm_f32
    akm, bkm = LAYOUTS[layout]
    _x3kg_env(monkeypatch)
    for ik, K in enumerate(KS):
        M, N = MN[(ik * 3 + nsplit - 1 + 5 * sorted(LAYOUTS).index(layout)) % len(MN)]
        A, B, ref, bound, _ = _case(M, N, K, akm, bkm)
        out, _ = gemm_f32(A, B, akm, bkm, tile=64, nsplit=nsplit)
        _check(out, ref, bound, K, "%s %dx%dx%d nsplit %d" % (layout, M, N, K, nsplit))
        again, _ = gemm_f32(A, B, akm, bkm, tile=64, nsplit=nsplit)
        np.testing.assert_array_equal(out, again)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_kloop_16wave_every_row_and_column_edge(layout, monkeypatch):
    """every (M, N) pair of the list at a K with a partial last K-tile (250) and at one inside a single K-tile (63), unsplit"""
    from ganmf_amd.engine import gemm_f32
    akm, bkm = LAYOUTS[layout]
    _x3kg_env(monkeypatch)
    for M, N in MN:
        for K in (63, 250):
            A, B, ref, bound, _ = _case(M, N, K, akm, bkm)
            out, _ = gemm_f32(A, B, akm, bkm, tile=64, nsplit=1)
            _check(out, ref, bound, K, "%s %dx%dx%d" % (layout, M, N, K))


@pytest.mark.parametrize("layout", ["NT", "NN"])
def test_kloop_16wave_gathered_rows(layout, monkeypatch):
    """GemmP::a_gather: the row list rides in the operand fetch; repeated ids, rows past M on the zero page, K-tile edges and splits"""
    from ganmf_amd.engine import gemm_f32_ex
    akm, bkm = LAYOUTS[layout]
    _x3kg_env(monkeypatch)
    for M, N, K, nsplit in [(65, 33, 65, 1), (63, 96, 250, 2), (128, 64, 129, 3), (1, 33, 64, 1), (65, 64, 993, 3)]:
        A, B, ref, bound, ids = _case(M, N, K, akm, bkm, rows=40)
        assert len(np.unique(ids)) < len(ids) or M == 1
        out, _ = gemm_f32_ex(A, B, akm, bkm, tile=64, nsplit=nsplit, a_gather=ids)
        _check(out, ref, bound, K, "%s gather %dx%dx%d nsplit %d" % (layout, M, N, K, nsplit))
        again, _ = gemm_f32_ex(A, B, akm, bkm, tile=64, nsplit=nsplit, a_gather=ids)
        np.testing.assert_array_equal(out, again)


@pytest.mark.parametrize("bkm", [False, True])
def test_kloop_64x32_kernel(bkm, monkeypatch, capfd):
    """gemm_bf16w_mfma (128-deep K-tiles, NT and NN): one whole K-tile, one K past it, and a long ragged K"""
    from ganmf_amd.engine import gemm_f32
    monkeypatch.setenv("GANMF_TUNE", "bf16w=2")
    monkeypatch.setenv("GANMF_DEBUG_PLAN", "1")
    for (M, N), K in zip([(65, 33), (128, 96), (63, 64)], [128, 129, 993]):
        A, B, ref, bound, _ = _case(M, N, K, False, bkm)
        capfd.readouterr()
        out, _ = gemm_f32(A, B, False, bkm)
        assert "64 x 32 tiles" in capfd.readouterr().err, "the planner did not select gemm_bf16w_mfma for %r" % ((M, N, K),)
        _check(out, ref, bound, K, "64x32 %s %dx%dx%d" % ("NN" if bkm else "NT", M, N, K))
        again, _ = gemm_f32(A, B, False, bkm)
        np.testing.assert_array_equal(out, again)


def test_kloop_4wave_tn_adam_epilogue(monkeypatch, capfd):
    """gemm_bf16s_body<64, 64, 32, true, true, 3> behind the fused-Adam epilogue (the weight-gradient launches' loop): one 32-deep K-tile,
    one and a half, and eight.  On zero state the first moment is m = fl(g * fl(1 - beta1)) -- the product, rounded once more (2^-24
    relative, the second term of the bound) -- and theta = -lr_t * m / (sqrt(v) + eps) with v = g^2 (1 - beta2) depends on g only through
    its sign and eps / |g|: checked to 2e-6 relative (seven fp32 roundings and the 1-ulp v_sqrt / v_rcp, 7e-7 together) where |g| is
    at least 1e-3 of sum |a||b|, i.e. far from a sign change."""
    from ganmf_amd.engine import gemm_f32_ex
    monkeypatch.setenv("GANMF_MFMA", "bf16x3")
    monkeypatch.delenv("GANMF_TUNE", raising=False)
    monkeypatch.setenv("GANMF_DEBUG_PLAN", "1")
    b1 = float(np.float32(1.0) - np.float32(0.9))
    b2 = float(np.float32(1.0) - np.float32(0.999))
    for (M, N), K in zip([(65, 96), (128, 33), (63, 64)], [32, 48, 256]):
        A, B, ref, bound, _ = _case(M, N, K, True, True)
        capfd.readouterr()
        theta, m, _ = gemm_f32_ex(A, B, True, True, tile=64, bk=32, adam=True)
        line = capfd.readouterr().err
        assert "tile 64" in line and " kg 1 " in line and "nsplit 1 " in line and "mfma bf16x3" in line, line      # the 4-wave staged kernel, unsplit
        err = np.abs(m - b1 * ref)
        worst = float((err / (bound + 1e-30)).max())
        print("TN adam %dx%dx%d: max err(m) / ((1 - beta1) sum|a||b|) = %.3e (bound %.3e)" % (M, N, K, worst / b1, 4e-7 * np.sqrt(K)))
        assert np.all(err <= b1 * 4e-7 * bound * np.sqrt(K) + 2.0 ** -24 * np.abs(b1 * ref) + 1e-30), worst
        big = np.abs(ref) >= 1e-3 * bound
        want = -1e-3 * (b1 * ref) / (np.sqrt(b2 * ref * ref) + 1e-8)
        assert big.sum() > 0.9 * big.size
        np.testing.assert_allclose(theta[big], want[big], rtol=2e-6, atol=0)
        theta2, m2, _ = gemm_f32_ex(A, B, True, True, tile=64, bk=32, adam=True)
        np.testing.assert_array_equal(m, m2)
        np.testing.assert_array_equal(theta, theta2)
