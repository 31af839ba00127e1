"""ganmf_als_half_sweep where tests/test_gpu_ials.py does not sample it: every tile-pair count of als_rows_mfma_kernel (<1>, <3>, <6>,
<9>, full and partly used), profile lengths on and around the gather tile of 32 entries, the mixes of empty, short and long rows inside
one workgroup of als_rows_small_kernel, and a call in which some rows have a system that is not positive definite and the others do.

Matrix: tests/helpers_ials.py edge_matrix (34 or 36 rows x 260).  Yardstick of every comparison of factors: the rule of
test_gpu_ials.py, device error against the float64 restatement <= FACTOR x e_f32, with e_f32 the LARGER error of two float32
restatements on the same inputs -- half_sweep (numpy's inverse) and half_sweep_cholesky (numpy's Cholesky and two substitutions).
Both are references, neither is the code under test; one sample of one of them is a noisy yardstick (the largest ratio of the first
suite is 3.39 of 4).  Every case prints its figures; those of the first run on an MI355X are in profiles/ials_parity.md."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import helpers_ials as H

pytestmark = pytest.mark.gpu

FACTOR = 4.0
N_COLS = 260
SCALINGS = [(1e-5, "linear"), (1e-2, "log")]
TILE_EDGE_LENGTHS = (31, 32, 33, 63, 64, 65, 96, 97, 200)


def _tensors(L, side):
    """(tensor id of the solved side, of the fixed side)"""
    return (L.T_USER_EMB, L.T_ITEM_EMB) if side == 0 else (L.T_ITEM_EMB, L.T_USER_EMB)


def _engine(n_rows, n_cols, k, side):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    n_users, n_items = (n_rows, n_cols) if side == 0 else (n_cols, n_rows)
    return Engine(n_users, n_items, k, 1, 1, model=L.MODEL_MF)


def _confidence(M, scaling):
    alpha, eps = (2.0, 1.0) if scaling == "linear" else (10.0, 0.5)
    return H.confidence(M, scaling, alpha, eps)


def _draw(n_rows, k, seed=None):
    """X0 and Y as tests/test_gpu_ials.py _sweep_case draws them"""
    rng = np.random.RandomState(k if seed is None else seed)
    X0 = rng.rand(n_rows, k).astype(np.float32)
    Y = (k ** -0.5 * rng.rand(N_COLS, k)).astype(np.float32)
    return X0, Y


def _sweep(eng, side, C, X0, Y, reg):
    """uploads C, X0 and Y, runs one half sweep of `side` and returns the solved side"""
    from ganmf_amd import _lib as L
    tx, ty = _tensors(L, side)
    eng.set_confidence(side, C)
    eng.set_tensor(tx, X0)
    eng.set_tensor(ty, Y)
    eng.als_half_sweep(side, reg)
    return eng.get_tensor(tx)


def _references(X0, Y, C, reg):
    """(float64 restatement, error of the inverse restatement in float32, error of the Cholesky restatement in float32)"""
    ref = H.half_sweep(X0, Y, C, reg, np.float64)
    e_inv = H.row_error(H.half_sweep(X0, Y, C, reg, np.float32), ref)
    e_chol = H.row_error(H.half_sweep_cholesky(X0, Y, C, reg, np.float32), ref)
    return ref, e_inv, e_chol


def _check_parity(X, X0, Y, C, reg, label, named_lengths=()):
    """the parity rule, the untouched empty rows, and per row of a length in `named_lengths` the same bound with the row's name"""
    ref, e_inv, e_chol = _references(X0, Y, C, reg)
    e_f32 = max(e_inv, e_chol)
    per_row = H.row_errors(X, ref)
    e_dev = float(per_row.max())
    print("ials edges %s: device %.3e  float32 inverse %.3e  float32 cholesky %.3e  ratio %.2f"
          % (label, e_dev, e_inv, e_chol, e_dev / e_f32 if e_f32 else np.inf))
    lengths = np.diff(C.indptr)
    if e_dev > FACTOR * e_f32:
        worst = int(per_row.argmax())
        B, _ = H.system_matrix(Y, C, worst, reg)
        print("ials edges %s: OVER %g: worst row %d, profile length %d, error %.3e, cond(B) %.3e, k eps cond(B) %.3e"
              % (label, FACTOR, worst, lengths[worst], per_row[worst], np.linalg.cond(B), Y.shape[1] * 2.0 ** -24 * np.linalg.cond(B)))
    assert np.isfinite(X).all()
    for u in np.flatnonzero(lengths == 0):
        assert X[u].tobytes() == X0[u].tobytes(), "row %d has no stored entry and must come back unchanged" % u
    assert e_dev <= FACTOR * e_f32, (label, e_dev, e_inv, e_chol)
    for n in named_lengths:
        for u in np.flatnonzero(lengths == n):
            print("ials edges %s: row %d of length %d: device %.3e (%.2f of e_f32)" % (label, u, n, per_row[u], per_row[u] / e_f32))
            assert per_row[u] <= FACTOR * e_f32, (label, "row %d, profile length %d" % (u, n), per_row[u], e_f32)


def _check_fixed_side_and_pads(eng, side, X, Y):
    """the fixed side keeps its bytes; the pad columns of the solved side stay zero (the scoring product reads the factor rows over
    their padded width)"""
    from ganmf_amd import _lib as L
    assert eng.get_tensor(_tensors(L, side)[1]).tobytes() == Y.tobytes()
    s = eng.scores(np.arange(X.shape[0]), transposed=(side == 1))
    want = X.astype(np.float64).dot(Y.astype(np.float64).T)
    bound = (np.abs(X).astype(np.float64).dot(np.abs(Y).astype(np.float64).T)).max()
    assert np.abs(s - want).max() <= 1e-5 * bound


def _edge_case(n_rows, k, reg, scaling, side, named_lengths):
    C = _confidence(H.edge_matrix(n_rows, N_COLS, 100 + k), scaling)
    X0, Y = _draw(n_rows, k)
    eng = _engine(n_rows, N_COLS, k, side)
    try:
        X = _sweep(eng, side, C, X0, Y, reg)
        _check_parity(X, X0, Y, C, reg, "%dx%d k=%d reg=%g %s side=%d" % (n_rows, N_COLS, k, reg, scaling, side), named_lengths)
        _check_fixed_side_and_pads(eng, side, X, Y)
    finally:
        eng.close()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("reg,scaling", SCALINGS)
@pytest.mark.parametrize("k", [96, 97, 128, 129, 160, 161, 192, 193, 224, 225])
def test_middle_ranks_against_float64(k, reg, scaling, side):
    """nt = 3 .. 8 tiles of 32: als_rows_mfma_kernel<3> with two and three slots used, <6> with four, five and six, <9> with seven
    and eight"""
    _edge_case(34, k, reg, scaling, side, ())


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("reg,scaling", SCALINGS)
@pytest.mark.parametrize("n_rows", [34, 36])
@pytest.mark.parametrize("k", [1, 8, 31, 32, 33, 64, 65])
def test_profile_and_workgroup_edges_against_float64(k, n_rows, reg, scaling, side):
    """k <= 32 the small kernel (four rows per workgroup; 34 and 36 rows leave two and no slot of the last one without a row),
    k > 32 the MFMA kernel; the rows whose length is on or next to a multiple of the gather tile are checked by name"""
    _edge_case(n_rows, k, reg, scaling, side, TILE_EDGE_LENGTHS)


@pytest.mark.parametrize("k", [8, 32, 33, 160])
def test_rows_with_the_same_profile_get_the_same_bytes_whatever_their_neighbours(k):
    """the six twin rows: wave slots 0 .. 3 of one workgroup of the small kernel, slot 0 beside a 64-entry row, slot 1 beside a
    200-entry row (whose tiles the twin's wave walks with zeros); then a lone twin among empty rows"""
    from ganmf_amd import _lib as L
    M = H.edge_matrix(34, N_COLS, 100 + k)
    C = _confidence(M, "linear")
    X0, Y = _draw(34, k)
    twins = list(H.EDGE_TWIN_ROWS)
    assert len(set(X0[u].tobytes() for u in twins)) == 6          # the rows' own factors differ: nothing of them may survive
    eng = _engine(34, N_COLS, k, 0)
    try:
        X = _sweep(eng, 0, C, X0, Y, 1e-3)
        assert np.isfinite(X).all()
        for u in twins[1:]:
            assert X[u].tobytes() == X[twins[0]].tobytes(), "twin rows %d and %d differ" % (twins[0], u)
        _check_parity(X, X0, Y, C, 1e-3, "34x%d k=%d reg=0.001 linear side=0 twins" % (N_COLS, k))      # equal AND the solutions
        # a matrix that holds one twin row only, in another wave slot of another workgroup
        lone = 6
        d = np.zeros((34, N_COLS), np.float32)
        lo, hi = M.indptr[twins[0]], M.indptr[twins[0] + 1]
        d[lone, M.indices[lo:hi]] = M.data[lo:hi]
        C1 = _confidence(sps.csr_matrix(d), "linear")
        assert np.array_equal(C1.data, C.data[lo:hi]) and np.array_equal(C1.indices, C.indices[lo:hi])
        X1 = _sweep(eng, 0, C1, X0, Y, 1e-3)
        assert X1[lone].tobytes() == X[twins[0]].tobytes()
        rest = np.arange(34) != lone
        assert X1[rest].tobytes() == X0[rest].tobytes()
        assert eng.get_tensor(L.T_ITEM_EMB).tobytes() == Y.tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("k", [2, 40])
def test_good_and_bad_rows_in_one_call_with_exact_answers(k):
    """Y[i] = e_(i mod k) over 2 k items, so G = 2 I exactly; reg = -2.5 and c = 3 everywhere.  A row holding one item of every
    coordinate has B = 1.5 I and b = 3: x = 2.  A row that misses coordinate k - 1 has B[k-1][k-1] = -0.5: it keeps its factors and
    is named, while the others are solved (k = 40: the pivot is in the second panel of the MFMA kernel)"""
    from ganmf_amd import _lib as L
    n_items = 2 * k
    Y = np.zeros((n_items, k), np.float32)
    Y[np.arange(n_items), np.arange(n_items) % k] = 1.0
    d = np.zeros((5, n_items), np.float32)
    d[1, :k] = 3.0
    d[2, :k - 1] = 3.0
    d[4, k:] = 3.0
    C = sps.csr_matrix(d)                                          # the confidences themselves
    X0 = np.random.RandomState(k).rand(5, k).astype(np.float32)
    ref = H.half_sweep(X0[[1, 4]], Y, C[[1, 4]], -2.5, np.float64)
    assert np.array_equal(ref, np.full((2, k), 2.0))
    eng = _engine(5, n_items, k, 0)
    try:
        eng.set_confidence(0, C)
        eng.set_tensor(L.T_USER_EMB, X0)
        eng.set_tensor(L.T_ITEM_EMB, Y)
        with pytest.raises(L.GanmfError, match=r"\(-4\).*row 2.*not positive definite"):
            eng.als_half_sweep(0, -2.5)
        X = eng.get_tensor(L.T_USER_EMB)
        print("ials edges exact k=%d: largest |x - 2| on the good rows %.3e" % (k, np.abs(X[[1, 4]] - 2.0).max()))
        assert np.isfinite(X).all()
        assert np.abs(X[[1, 4]] - 2.0).max() <= 4 * k * 2.0 ** -24 * 2.0
        for u in (0, 2, 3):
            assert X[u].tobytes() == X0[u].tobytes(), u
        assert eng.get_tensor(L.T_ITEM_EMB).tobytes() == Y.tobytes()
        eng.als_half_sweep(0, 1e-3)                                # the flag is cleared: every row has a positive definite system now
        X2 = eng.get_tensor(L.T_USER_EMB)
        assert np.isfinite(X2).all()
        want = H.half_sweep(X, Y, C, 1e-3, np.float64)
        assert H.row_error(X2, want) <= 4 * k * 2.0 ** -24        # B is diagonal with entries 2.001 and 4.001: cond(B) = 2
        assert X2[0].tobytes() == X0[0].tobytes() and X2[3].tobytes() == X0[3].tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("k,zero", [(20, 10), (40, 3), (40, 35), (100, 99)])
def test_a_zero_pivot_in_each_position(k, zero):
    """reg = 0 and one column of Y all zero: row and column `zero` of every B are exact zeros (every product that feeds them has a
    zero factor), so pivot `zero` is 0 in every row -- in the small kernel, in the first panel, a later panel, and as the very last
    pivot.  No row is written, the first row with an entry is named, and the next call starts with the flags cleared"""
    from ganmf_amd import _lib as L
    C = _confidence(H.edge_matrix(34, N_COLS, 100 + k), "linear")
    X0, Y = _draw(34, k)
    Yz = Y.copy()
    Yz[:, zero] = 0.0
    eng = _engine(34, N_COLS, k, 0)
    try:
        eng.set_confidence(0, C)
        eng.set_tensor(L.T_USER_EMB, X0)
        eng.set_tensor(L.T_ITEM_EMB, Yz)
        with pytest.raises(L.GanmfError, match=r"\(-4\).*row 1:.*not positive definite"):
            eng.als_half_sweep(0, 0.0)
        assert eng.get_tensor(L.T_USER_EMB).tobytes() == X0.tobytes()
        assert eng.get_tensor(L.T_ITEM_EMB).tobytes() == Yz.tobytes()
        eng.set_tensor(L.T_ITEM_EMB, Y)
        eng.als_half_sweep(0, 1e-2)
        X = eng.get_tensor(L.T_USER_EMB)
        _check_parity(X, X0, Y, C, 1e-2, "34x%d k=%d reg=0.01 linear side=0 after a zero pivot %d" % (N_COLS, k, zero))
        _check_fixed_side_and_pads(eng, 0, X, Y)
    finally:
        eng.close()
