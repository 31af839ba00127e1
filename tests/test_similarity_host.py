"""CPU checks of the helpers behind the prediction-similarity tests (tests/helpers_similarity.py): the float32 restatement is the
function the reference calls (AblationStudy.py:88-92: sklearn's cosine_similarity), the fp64 oracle's mean / std from the sums of
d = c - 1 are np.mean / np.std of its matrix, and the bin rule of the pooled block means."""
import numpy as np
import pytest

from tests.helpers_similarity import bin_edges, cosine32, oracle64, pooled_means, restatement32, stats_from_sums

ULP1 = 2.0 ** -23      # float32 spacing at 1


def _factors(seed, n, W, k):
    rng = np.random.RandomState(seed)
    return rng.randn(n, k).astype(np.float32), rng.randn(W, k).astype(np.float32)


def test_restatement_is_sklearn_cosine_similarity():
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    rows, cols = _factors(0, 129, 257, 40)
    rows[5] = 0.0      # an all-zero score row: sklearn's normalize leaves it zero
    rows[77] = 0.0
    s = rows @ cols.T
    want = pairwise.cosine_similarity(s)
    got = cosine32(s)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 4 * ULP1
    assert np.all(got[5] == 0) and np.all(got[:, 5] == 0) and got[77, 77] == 0 and np.all(want[5] == 0) and want[77, 77] == 0
    assert np.array_equal(restatement32(rows, cols), got)


@pytest.mark.parametrize("n,W,k,zero", [(1, 70, 8, False), (65, 70, 8, True), (200, 257, 40, True)])
def test_oracle_statistics_are_numpy_mean_and_std(n, W, k, zero):
    rows, cols = _factors(1, n, W, k)
    if zero:
        rows[n // 2] = 0.0
    # a nearly collapsed model as well: every row close to one profile
    for r in (rows, (rows[:1] + 1e-3 * rows).astype(np.float32)):
        o = oracle64(r, cols)
        c = o["matrix"]
        assert o["zero_rows"] == int(zero and r is rows)
        assert abs(o["mean"] - np.mean(c)) <= 1e-13
        assert abs(o["std"] - np.std(c)) <= 1e-9 + 1e-7 * np.std(c)
        assert stats_from_sums(o["sum_d"], o["sum_d2"], n) == (o["mean"], o["std"])


@pytest.mark.parametrize("n,pool", [(200, 7), (10, 3), (65, 64), (129, 2), (5, 5), (9, 1)])
def test_bin_rule(n, pool):
    rng = np.random.RandomState(n * 31 + pool)
    c = rng.randn(n, n)
    bins = [i * pool // n for i in range(n)]
    edges = bin_edges(n, pool)
    assert edges[0] == 0 and edges[-1] == n and np.all(np.diff(edges) >= 1)
    for b in range(pool):
        assert [i for i in range(n) if bins[i] == b] == list(range(edges[b], edges[b + 1]))
    want = np.empty((pool, pool))
    for a in range(pool):
        for b in range(pool):
            want[a, b] = np.mean([c[i, j] for i in range(edges[a], edges[a + 1]) for j in range(edges[b], edges[b + 1])])
    got = pooled_means(c, pool)
    assert np.abs(got - want).max() <= 1e-12
    if pool == 1:
        assert abs(got[0, 0] - c.mean()) <= 1e-12
    if pool == n:
        assert np.abs(got - c).max() <= 1e-15
