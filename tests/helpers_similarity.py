"""Shared pieces of the prediction-similarity checks (not a conftest: imported by the modules that use them).

Two restatements of the computation under the reference's collapse study (AblationStudy.py:88-92,113-117:
sklearn.metrics.pairwise.cosine_similarity of all predictions, np.mean and np.std of the matrix):

  * oracle64: everything in float64 from the factors -- scores, normalisation with sklearn's zero-norm rule (a zero norm is
    replaced by 1, so the row stays zero and its similarity with every row, itself included, is 0), the Gram product, the mean
    and the population standard deviation formed from d = c - 1, and the pooled block means;
  * restatement32: the reference's own sequence in float32 -- float32 scores, float32 row norms, float32 divide, float32 matrix
    product -- whose distance from oracle64 is the yardstick of the device's (tests/test_gpu_similarity.py)."""
import numpy as np


def bin_edges(n, pool):
    """row i belongs to bin i * pool // n: first row of every bin, and n"""
    return np.array([-((-b * n) // pool) for b in range(pool + 1)], dtype=np.int64)


def pooled_means(c, pool):
    """[pool, pool] block means of the square matrix c under the bin rule, in float64"""
    n = c.shape[0]
    bins = (np.arange(n, dtype=np.int64) * pool) // n
    onehot = np.zeros((pool, n), dtype=np.float64)
    onehot[bins, np.arange(n)] = 1.0
    counts = onehot.sum(axis=1)
    return (onehot @ c.astype(np.float64) @ onehot.T) / np.outer(counts, counts)


def stats_from_sums(sum_d, sum_d2, n):
    """(mean, population std) of c from the sums of d = c - 1 and d^2 over the n^2 pairs"""
    md = sum_d / (float(n) * n)
    return 1.0 + md, float(np.sqrt(max(sum_d2 / (float(n) * n) - md * md, 0.0)))


def oracle64(rows, cols):
    """rows [n, k], cols [W, k] (any float dtype) -> dict(matrix, sum_d, sum_d2, mean, std, zero_rows), all float64"""
    s = rows.astype(np.float64) @ cols.astype(np.float64).T
    norm = np.sqrt((s * s).sum(axis=1))
    zero = norm == 0.0
    norm[zero] = 1.0
    sh = s / norm[:, None]
    c = sh @ sh.T
    d = c - 1.0
    n = c.shape[0]
    mean, std = stats_from_sums(d.sum(), (d * d).sum(), n)
    return dict(matrix=c, sum_d=float(d.sum()), sum_d2=float((d * d).sum()), mean=mean, std=std, zero_rows=int(zero.sum()))


def cosine32(s):
    """float32 scores -> [n, n] float32 similarities by the reference's sequence: float32 row norms, divide, matrix product"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    norm = np.sqrt(np.einsum("ij,ij->i", s, s)).astype(np.float32)
    norm[norm == 0.0] = np.float32(1.0)
    sh = (s / norm[:, None]).astype(np.float32)
    return sh @ sh.T


def restatement32(rows, cols):
    """the reference's sequence in float32 from the factors: float32 scores, then cosine32"""
    return cosine32(rows.astype(np.float32) @ cols.astype(np.float32).T)


def restatement32_stats(c32):
    """np.mean / np.std as the reference takes them of its float32 matrix"""
    return float(np.mean(c32)), float(np.std(c32))
