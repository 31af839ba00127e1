"""Device memory of the library, counted by the library itself (ganmf_live_device_bytes: csrc/lib/devmem.inc adds every allocation
and subtracts every free).  Lifetimes: every kind of handle and trainer gives back exactly what it took.  Replacements: a second
upload or fit on a handle leaves what a fresh handle holds after that call alone, and scores the same bits.  Empty shapes upload
and score.  Everything at U = 300, N = 500, k = 16."""
import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

U, N, K = 300, 500, 16
IDS = np.arange(U)


def _live():
    from ganmf_amd import _lib as L
    return int(L.load_library().ganmf_live_device_bytes())


def _urm(seed=0, density=0.05):
    rng = np.random.RandomState(seed)
    m = sps.csr_matrix((rng.rand(U, N) < density).astype(np.float32))
    m.sort_indices()
    return m


def _transpose(m):
    t = m.tocsc()
    t.sort_indices()
    return sps.csr_matrix((t.data, t.indices, t.indptr), shape=(m.shape[1], m.shape[0]))


def _engine(model, k=K, e=24, batch=64, **kw):
    from ganmf_amd.engine import Engine
    return Engine(U, N, k, e, batch, model=model, **kw)


def _sides(eng, urm):
    eng.set_confidence(0, urm)
    eng.set_confidence(1, _transpose(urm))


def _use(eng, urm, seed=5):
    """what every lifetime ends with: scores, recommend, and one evaluate_full with seen, test, ratings and weights set"""
    rng = np.random.RandomState(seed)
    test = sps.csr_matrix((rng.rand(U, N) < 0.02).astype(np.float32))
    test.sort_indices()
    eng.set_seen(urm)
    s = eng.scores(IDS)
    assert s.shape == (U, N)
    eng.recommend(IDS, 5)
    eng.set_test(test, np.ones(test.nnz))
    eng.set_test_ratings(test.data)
    eng.set_eval_item_weights(np.ones(N), np.ones(N))
    eng.evaluate_full(IDS, [5], 1.0 / np.log2(np.arange(5) + 2.0), np.ones((U, 5)))
    return s


# ---- lifetimes: one case per kind of handle and trainer ---------------------------------------------------------------------------
def _fit_ganmf(urm):
    from ganmf_amd import _lib as L
    eng = _engine(L.MODEL_GANMF)
    eng.set_urm(urm)
    eng.train_epoch(np.random.RandomState(1).permutation(U), 1, 1)
    eng.snapshot_best()
    return eng


def _fit_disganmf(urm):
    from ganmf_amd import _lib as L
    eng = _engine(L.MODEL_DISGANMF, d_layers=2, d_act="tanh")
    eng.set_urm(urm)
    eng.train_epoch(np.random.RandomState(1).permutation(U), 1, 1)
    return eng


def _mf(urm):
    from ganmf_amd import _lib as L
    eng = _engine(L.MODEL_MF, e=1, batch=1)
    _sides(eng, urm)
    rng = np.random.RandomState(2)
    eng.set_tensor(L.T_USER_EMB, rng.rand(U, K).astype(np.float32))
    eng.set_tensor(L.T_ITEM_EMB, rng.rand(N, K).astype(np.float32))
    return eng


def _fit_als(urm):
    eng = _mf(urm)
    eng.als_half_sweep(0, 0.1)
    eng.als_half_sweep(1, 0.1)
    return eng


def _fit_puresvd(urm, n_random=24):
    eng = _mf(urm)
    eng.pure_svd(np.random.RandomState(3).randn(min(U, N), n_random).astype(np.float32), 2)
    return eng


def _fit_nmf_mu(urm):
    from ganmf_amd import _lib as L
    eng = _mf(urm)
    eng.nmf_mu(L.NMF_FROBENIUS, 2)
    eng.nmf_mu(L.NMF_KULLBACK_LEIBLER, 1)
    return eng


def _fit_nmf_cd(urm):
    eng = _mf(urm)
    eng.nmf_cd(np.stack([np.stack([np.random.RandomState(4).permutation(K)] * 2)] * 2))
    return eng


def _fit_mf_sgd(algorithm):
    def fit(urm):
        from ganmf_amd import _lib as L
        eng = _engine(L.MODEL_MF, e=1, batch=1)
        rng = np.random.RandomState(6)
        eng.mf_sgd_init(algorithm, urm, rng.rand(U, K), rng.rand(N, K), seed=1)
        eng.mf_sgd_epochs(1, batch_size=1000 if algorithm == "MF_BPR" else 1)
        eng.mf_sgd_publish()
        return eng
    return fit


def _itemsim(urm):
    from ganmf_amd import _lib as L
    eng = _engine(L.MODEL_ITEMSIM, k=1, e=1, batch=1)
    _sides(eng, urm)
    return eng


def _fit_itemknn(urm):
    from ganmf_amd import _lib as L
    eng = _itemsim(urm)
    eng.itemknn_fit(L.ITEMKNN_RAW, 10)
    return eng


def _fit_userknn(urm):
    from ganmf_amd import _lib as L
    eng = _itemsim(urm)
    eng.userknn_fit(L.ITEMKNN_RAW, 10)
    return eng


def _fit_p3(urm):
    eng = _itemsim(urm)
    eng.p3_fit(10, np.ones(N, dtype=np.float32))
    return eng


def _fit_slim(urm):
    eng = _itemsim(urm)
    eng.slim_bpr_init(symmetric=True, sgd_mode="adam", seed=1)
    eng.slim_bpr_epochs(1)
    eng.slim_bpr_finish(10)
    return eng


def _k_rows(urm):
    return np.minimum(N - np.diff(urm.indptr), 20).astype(np.int32)


def _cfgan(urm, init=True):
    from ganmf_amd import _lib as L
    eng = _engine(L.MODEL_CFGAN, k=1, e=8, batch=64, m=0.0, recon_coefficient=0.0, d_layers=1, d_act="linear")
    eng.set_urm(urm)
    if init:
        eng.cfgan_init(8, 1, "linear", 64, 64, "ZP", 0.1, 1, _k_rows(urm))
    return eng


def _fit_cfgan(urm):
    eng = _cfgan(urm)
    eng.cfgan_epoch(0)
    return eng


def _caae(urm, init=True):
    from ganmf_amd import _lib as L
    eng = _engine(L.MODEL_CAAE, e=1, batch=1)
    eng.set_urm(urm)
    if init:
        eng.caae_init(8, 1, 2048, 32, 4, 0.5, 1e-4, 1e-3, 1, _k_rows(urm))
    return eng


def _fit_caae(urm):
    eng = _caae(urm)
    eng.caae_epoch(0)
    return eng


LIFETIMES = {
    "ganmf": _fit_ganmf, "disganmf": _fit_disganmf, "als": _fit_als, "puresvd": _fit_puresvd, "nmf_mu": _fit_nmf_mu,
    "nmf_cd": _fit_nmf_cd, "mf_bpr": _fit_mf_sgd("MF_BPR"), "funk_svd": _fit_mf_sgd("FUNK_SVD"), "itemknn": _fit_itemknn,
    "userknn": _fit_userknn, "p3": _fit_p3, "slim_bpr": _fit_slim, "cfgan": _fit_cfgan, "caae": _fit_caae,
}


@pytest.mark.parametrize("kind", sorted(LIFETIMES))
def test_a_lifetime_gives_back_every_byte(kind):
    urm = _urm()
    before = _live()
    eng = LIFETIMES[kind](urm)
    assert _live() > before
    _use(eng, urm)
    eng.close()
    assert _live() == before, "%s: %d bytes are still counted live after close()" % (kind, _live() - before)


# ---- replacements: the second call leaves what a fresh handle holds after that call alone ----------------------------------------
def _same_as_fresh(twice, fresh, urm_for_scores=None):
    """both engines built from the same live-byte count: their totals and the bits of their scores agree"""
    base = _live()
    a = twice()
    held_a = _live() - base
    b = fresh()
    held_b = _live() - base - held_a
    try:
        assert held_a == held_b, "%d bytes after the second call, %d on a fresh handle" % (held_a, held_b)
        if urm_for_scores is not None:
            assert np.array_equal(a.scores(IDS).view(np.uint32), b.scores(IDS).view(np.uint32))
    finally:
        a.close()
        b.close()
    assert _live() == base


def test_set_urm_twice(monkeypatch):
    """sparse enough for the CSC twin the first time (GANMF_SPARSE_D = 1), dense the second: the twin and its row buffer are gone"""
    from ganmf_amd import _lib as L
    sparse, dense = _urm(1, 0.004), _urm(2, 0.05)
    rng = np.random.RandomState(0)
    Ue, V = rng.randn(U, K).astype(np.float32), rng.randn(N, K).astype(np.float32)

    def make(first):
        eng = _engine(L.MODEL_GANMF)
        if first:
            monkeypatch.setenv("GANMF_SPARSE_D", "1")
            held = _live()
            eng.set_urm(sparse)
            # URM: (U + 1) row pointers, nnz indices and values; the CSC twin: (N + 1) column pointers, nnz rows and values; sp_rows on top
            assert _live() - held > 8 * (U + 1) + 8 * (N + 1) + 16 * sparse.nnz
        monkeypatch.setenv("GANMF_SPARSE_D", "0")
        eng.set_urm(dense)
        eng.set_tensor(L.T_USER_EMB, Ue)
        eng.set_tensor(L.T_ITEM_EMB, V)
        return eng
    _same_as_fresh(lambda: make(True), lambda: make(False), True)


def test_seen_test_and_candidates_twice():
    from ganmf_amd import _lib as L
    big, small = _urm(3, 0.08), _urm(4, 0.02)
    rng = np.random.RandomState(0)
    Ue, V = rng.randn(U, K).astype(np.float32), rng.randn(N, K).astype(np.float32)

    def make(first):
        eng = _engine(L.MODEL_MF, e=1, batch=1)
        eng.set_tensor(L.T_USER_EMB, Ue)
        eng.set_tensor(L.T_ITEM_EMB, V)
        for m in ([big, small] if first else [small]):
            eng.set_seen(m)
            eng.set_test(m, np.ones(m.nnz))
            eng.set_test_ratings(m.data)
            eng.set_candidates(m)
        eng.set_candidates(None)
        return eng
    _same_as_fresh(lambda: make(True), lambda: make(False), True)


def test_als_confidence_twice_per_side():
    from ganmf_amd import _lib as L
    big, small = _urm(3, 0.08), _urm(4, 0.02)
    rng = np.random.RandomState(0)
    Ue, V = rng.rand(U, K).astype(np.float32), rng.rand(N, K).astype(np.float32)

    def make(first):
        eng = _engine(L.MODEL_MF, e=1, batch=1)
        eng.set_tensor(L.T_USER_EMB, Ue)
        eng.set_tensor(L.T_ITEM_EMB, V)
        for m in ([big, small] if first else [small]):
            _sides(eng, m)
        eng.als_half_sweep(0, 0.1)
        return eng
    _same_as_fresh(lambda: make(True), lambda: make(False), True)


def test_item_similarity_then_a_userknn_fit():
    from ganmf_amd import _lib as L
    urm = _urm()
    W = sps.random(N, N, density=0.01, format="csr", dtype=np.float32, random_state=7)

    def make(first):
        eng = _itemsim(urm)
        if first:
            eng.set_item_similarity(W)
        eng.userknn_fit(L.ITEMKNN_RAW, 10)
        return eng
    _same_as_fresh(lambda: make(True), lambda: make(False), True)


def test_pure_svd_with_a_wider_n_random():
    urm = _urm()

    def make(first):
        eng = _mf(urm)
        om = np.random.RandomState(3).randn(min(U, N), 100).astype(np.float32)      # (the panels are a multiple of 64 columns wide)
        if first:
            eng.pure_svd(om[:, :40], 1)
        eng.pure_svd(om, 1)
        return eng
    _same_as_fresh(lambda: make(True), lambda: make(False), True)


@pytest.mark.parametrize("model", ["cfgan", "caae"])
def test_init_twice(model):
    """the second _init is refused ("once per engine") and changes nothing"""
    from ganmf_amd._lib import GanmfError
    urm = _urm()
    build = _cfgan if model == "cfgan" else _caae

    def twice():
        eng = build(urm)
        with pytest.raises(GanmfError, match="initialised already"):
            (eng.cfgan_init(8, 1, "linear", 64, 64, "ZP", 0.1, 1, _k_rows(urm)) if model == "cfgan" else
             eng.caae_init(8, 1, 2048, 32, 4, 0.5, 1e-4, 1e-3, 1, _k_rows(urm)))
        return eng
    _same_as_fresh(twice, lambda: build(urm), True)


# ---- empty shapes -----------------------------------------------------------------------------------------------------------------
def test_empty_last_row_and_empty_test_matrix():
    from ganmf_amd import _lib as L
    urm = _urm().tolil()
    urm[U - 1, :] = 0
    urm = sps.csr_matrix(urm)
    urm.eliminate_zeros()
    urm.sort_indices()
    assert urm.indptr[-1] == urm.indptr[-2]
    before = _live()
    eng = _engine(L.MODEL_GANMF)
    eng.set_urm(urm)
    eng.set_seen(urm)
    rng = np.random.RandomState(0)
    Ue, V = rng.randn(U, K).astype(np.float32), rng.randn(N, K).astype(np.float32)
    eng.set_tensor(L.T_USER_EMB, Ue)
    eng.set_tensor(L.T_ITEM_EMB, V)
    s = eng.scores(IDS)
    ref = Ue.astype(np.float64) @ V.astype(np.float64).T
    assert np.abs(s - ref).max() <= 1e-4 * np.abs(ref).max()
    items, _ = eng.recommend(IDS, 5)
    assert items.shape == (U, 5)
    empty = sps.csr_matrix((U, N), dtype=np.float32)
    eng.set_test(empty, np.ones(0))
    eng.set_test_ratings(np.ones(0, dtype=np.float32))
    eng.set_eval_item_weights(np.ones(N), np.ones(N))
    eng.evaluate_full(IDS, [5], np.ones(5), np.ones((U, 5)))
    eng.close()
    assert _live() == before
