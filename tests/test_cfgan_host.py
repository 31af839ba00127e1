"""CFGAN on the host: the numpy restatement's gradients against torch.autograd in float64, the host mask sampler against a literal
loop of np.random.choice, the bit order of the mask planes, and the restatement of the device sampler."""
import numpy as np
import pytest
import scipy.sparse as sps

from ganmf_amd.CFGAN import (draw_masks_numpy, init_weights, mask_size, non_interactions, pack_mask_rows, unpack_mask_rows)
from tests import helpers_cfgan as H


def _torch_losses(w, c, M, ZR, d_act, g_act, d_reg, g_reg, coef):
    import torch
    torch.set_default_dtype(torch.float64)
    acts = {"linear": lambda z: z, "tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid}
    P = {k: [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in v] for k, v in w.items()}

    def mlp(key, x, a):
        for l in range(len(P[key]) // 2 - 1):
            x = acts[a](x @ P[key][2 * l] + P[key][2 * l + 1])
        return x @ P[key][-2] + P[key][-1]
    c, M, ZR = (torch.tensor(np.asarray(a, np.float64)) for a in (c, M, ZR))
    fake = mlp("G", c, g_act)
    gout = fake * M
    d_real = mlp("D", torch.cat([c, c], 1), d_act)
    d_fake = mlp("D", torch.cat([c, gout], 1), d_act)
    sp = torch.nn.functional.softplus
    l2 = lambda key: sum(0.5 * (p * p).sum() for p in P[key])
    d_loss = sp(-d_real).mean() + sp(d_fake).mean() + d_reg * l2("D")
    g_loss = sp(-d_fake).mean() + g_reg * l2("G") + coef * (fake * fake * ZR).sum(1).mean()
    gd = torch.autograd.grad(d_loss, P["D"], retain_graph=True)
    gg = torch.autograd.grad(g_loss, P["G"])
    return d_loss.item(), [g.numpy() for g in gd], g_loss.item(), [g.numpy() for g in gg]


@pytest.mark.parametrize("d_act,g_act,dl,gl", [("linear", "linear", 1, 1), ("tanh", "sigmoid", 2, 3), ("relu", "tanh", 3, 1),
                                                ("sigmoid", "relu", 1, 2)])
def test_restatement_gradients_match_autograd(d_act, g_act, dl, gl):
    pytest.importorskip("torch")
    rng = np.random.RandomState(3)
    B, I = 7, 13
    c = (rng.rand(B, I) < 0.3) * rng.randint(1, 6, size=(B, I)).astype(np.float64)
    PM = ((rng.rand(B, I) < 0.3) & (c == 0)).astype(np.float64)
    ZR = ((rng.rand(B, I) < 0.3) & (c == 0)).astype(np.float64)
    w = init_weights(5, I, 6, dl, 5, gl)
    w = {k: [a.astype(np.float64) * 3 for a in v] for k, v in w.items()}
    ref = H.CFGANRef(w, d_act=d_act, g_act=g_act, d_reg=0.01, g_reg=0.02, zr_coefficient=0.3)
    dloss, gd = ref.d_grads(c, c + PM)
    gloss, gg = ref.g_grads(c, c + PM, ZR)
    tdl, tgd, tgl, tgg = _torch_losses(w, c, c + PM, ZR, d_act, g_act, 0.01, 0.02, 0.3)
    assert abs(dloss - tdl) <= 1e-12 * max(1.0, abs(tdl)) and abs(gloss - tgl) <= 1e-12 * max(1.0, abs(tgl))
    for got, want in list(zip(gd, tgd)) + list(zip(gg, tgg)):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_mask_size_goes_through_a_c_float():
    assert mask_size(10, 0.7) == 6 and mask_size(20, 0.7) == 13 and mask_size(100, 0.7) == 69
    assert mask_size(10, 0.9) == 8 and mask_size(20, 0.9) == 17 and mask_size(100, 0.9) == 89
    for n in (10, 20, 100):
        for r in (0.1, 0.3, 0.5):
            assert mask_size(n, r) == int(round(n * r))
    assert mask_size(10, 0.0) == 0 and mask_size(10, 1.0) == 10


def _urm(rows=9, I=14, seed=2):
    rng = np.random.RandomState(seed)
    d = (rng.rand(rows, I) < 0.3).astype(np.float32)
    d[0] = 0
    d[0, :4] = 1          # 10 non-interactions
    d[1] = 1              # full profile
    d[2] = 0              # empty profile
    return sps.csr_matrix(d)


@pytest.mark.parametrize("scheme", ["ZR", "PM", "ZP"])
@pytest.mark.parametrize("ratio", [0.7, 0.3])
def test_draw_masks_numpy_is_the_literal_loop(scheme, ratio):
    urm = _urm()
    free = non_interactions(urm)
    np.random.seed(11)
    zr, pm = draw_masks_numpy(urm, scheme, ratio)
    np.random.seed(11)
    want_zr, want_pm = np.zeros(urm.shape, bool), np.zeros(urm.shape, bool)
    r32 = float(np.float32(ratio))
    for u in range(urm.shape[0]):      # compute_masks: zr_ratio sizes BOTH draws, through a C float
        if scheme in ("ZP", "ZR"):
            want_zr[u, np.random.choice(free[u], size=int(len(free[u]) * r32), replace=False)] = True
        if scheme in ("ZP", "PM"):
            want_pm[u, np.random.choice(free[u], size=int(len(free[u]) * r32), replace=False)] = True
    assert np.array_equal(zr, want_zr) and np.array_equal(pm, want_pm)
    assert len(free[0]) == 10
    if ratio == 0.7:
        assert (zr[0].sum() if scheme != "PM" else pm[0].sum()) == 6
    dense = urm.toarray() != 0
    assert not (zr & dense).any() and not (pm & dense).any()
    assert zr.any() == (scheme != "PM") and pm.any() == (scheme != "ZR")


def test_draw_masks_numpy_takes_a_private_stream():
    urm = _urm()
    a = draw_masks_numpy(urm, "ZP", 0.5, rng=np.random.RandomState(4))
    np.random.seed(4)
    b = draw_masks_numpy(urm, "ZP", 0.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        draw_masks_numpy(urm, "XX", 0.5)


@pytest.mark.parametrize("I", [1, 31, 32, 33, 64, 70])
def test_pack_unpack_bit_order(I):
    rng = np.random.RandomState(I)
    dense = rng.rand(5, I) < 0.4
    w = pack_mask_rows(dense)
    assert w.dtype == np.uint32 and w.shape == (5, (I + 31) // 32)
    for r in range(5):
        for j in range(I):
            assert bool((int(w[r, j >> 5]) >> (j & 31)) & 1) == bool(dense[r, j])
    if I % 32:
        assert not (w[:, -1] >> np.uint32(I % 32)).any()      # tail bits are 0
    assert np.array_equal(unpack_mask_rows(w, I), dense)
    one = np.zeros((1, 40), bool)
    one[0, 33] = True
    assert pack_mask_rows(one).tolist() == [[0, 2]]


@pytest.mark.parametrize("scheme", ["ZR", "PM", "ZP"])
def test_sampler_restatement_sizes_and_eligibility(scheme):
    urm = H.make_case(70)
    lens = np.diff(urm.indptr)
    dense = urm.toarray() != 0
    for ratio in (0.0, 0.05, 0.7, 1.0):
        k = [mask_size(70 - int(n), ratio) for n in lens]
        zr, pm = H.sampler_masks(urm, scheme, k, seed=7, epoch=3)
        for plane, used in ((zr, scheme != "PM"), (pm, scheme != "ZR")):
            assert not (plane & dense).any()
            assert np.array_equal(plane.sum(axis=1), np.array(k) if used else np.zeros(len(k), int))
        again = H.sampler_masks(urm, scheme, k, seed=7, epoch=3)
        assert np.array_equal(zr, again[0]) and np.array_equal(pm, again[1])
    k = [mask_size(70 - int(n), 0.5) for n in lens]
    a, b = H.sampler_masks(urm, "ZP", k, 7, 3), H.sampler_masks(urm, "ZP", k, 7, 4)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[0], a[1])


def test_sampler_mix_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 (the published test vector of the generator the key function comes from)
    assert H.mix(0) == 0xE220A8397B1DCDAF
    assert H.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    z = np.array([0, 0x9E3779B97F4A7C15], dtype=np.uint64)
    assert [int(v) for v in H.mix_np(z)] == [H.mix(0), H.mix(0x9E3779B97F4A7C15)]
    keys = H.sampler_keys(1, 2, 1, 5, np.arange(4))
    base = H.mix(H.mix(H.mix(1) ^ 2) ^ 1)
    assert [int(v) for v in keys] == [H.mix(base ^ ((5 << 32) | j)) >> 32 for j in range(4)]


def test_ties_go_to_the_smaller_column(monkeypatch):
    monkeypatch.setattr(H, "sampler_keys", lambda seed, epoch, plane, row, cols: np.array([5, 1, 5, 5, 9], dtype=np.uint32)[:len(cols)])
    assert sorted(H.sampler_row(0, 0, 0, 0, [10, 11, 12, 13, 14], 3)) == [10, 11, 12]
