"""Shared pieces of the discriminator-inference tests (tests/test_discriminator_host.py, tests/test_gpu_discriminator.py).

Two restatements of what ganmf_discriminate returns, built on the oracle classes' own lines (GANMFOracle.generator and the three
lines of GANMFOracle.autoencoder; DisGANMFOracle.discriminator):
  oracle64       float64 throughout: the reference value;
  restatement32  float32 throughout: the reference's own sequence in the reference's dtype.  Its distance from oracle64 on the same
                 inputs is the yardstick of the bound: the device may deviate from oracle64 by max(4 x that distance, floor).
Inputs are of one kind everywhere: Glorot weights + 0.05 randn (biases 0.05 randn), 5 %-dense rows with one empty and one full row.
"""
import numpy as np
import scipy.sparse as sps

from oracle.ganmf_oracle import DisGANMFOracle, GANMFOracle, glorot_uniform

EPS32 = 2.0 ** -23
DOMAIN = 300          # rows of the training matrix in every shape case
K_FACTORS = 8


def make_urm(num_users, num_items, seed, binary=True, density=0.05):
    """[num_users, num_items] CSR float32: `density` random entries per row, row 0 empty, row 1 with all num_items entries stored;
    binary=False: stored values 0.5 .. 5 in steps of 0.5 instead of 1"""
    rng = np.random.RandomState(seed)
    m = (rng.rand(num_users, num_items) < density).astype(np.float32)
    m[0, :] = 0.0
    m[1, :] = 1.0
    if not binary:
        m *= rng.randint(1, 11, size=m.shape).astype(np.float32) * 0.5
    return sps.csr_matrix(m)


def make_ids(num_users, n, seed):
    """n row ids: a shuffled subset of the domain that starts from the empty row 0 and the full row 1, its first id repeated at the
    end (n = 1: the full row alone)"""
    rng = np.random.RandomState(seed)
    pool = np.concatenate([[0, 1], 2 + rng.permutation(num_users - 2)])
    ids = pool[:n - 1].copy() if n > 1 else pool[1:2].copy()
    rng.shuffle(ids)
    return np.concatenate([ids, ids[:1]])[:n].astype(np.int32)


def ganmf_weights(num_users, num_items, k, e, seed):
    rng = np.random.RandomState(seed)
    noisy = lambda shape: (glorot_uniform(rng, shape) + 0.05 * rng.randn(*shape)).astype(np.float32)
    return {"We": noisy((num_items, e)), "be": (0.05 * rng.randn(e)).astype(np.float32),
            "Wd": noisy((e, num_items)), "bd": (0.05 * rng.randn(num_items)).astype(np.float32),
            "U": noisy((num_users, k)), "V": noisy((num_items, k))}


def disganmf_weights(num_users, num_items, k, layers, nodes, seed):
    """layer_0/kernel is [num_items + 1, nodes] with row 0 multiplying float(uid) (DisGANMF.py:59); that row is scaled by
    1 / num_users so that the uid term is of the size of the other terms"""
    rng = np.random.RandomState(seed)
    noisy = lambda shape: (glorot_uniform(rng, shape) + 0.05 * rng.randn(*shape)).astype(np.float32)
    w, fan_in = {}, num_items + 1
    for l in range(layers):
        w["W%d" % l] = noisy((fan_in, nodes))
        w["b%d" % l] = (0.05 * rng.randn(nodes)).astype(np.float32)
        fan_in = nodes
    w["W0"][0] /= np.float32(num_users)
    w["Wo"] = noisy((fan_in, 1))
    w["bo"] = (0.05 * rng.randn(1)).astype(np.float32)
    w["U"], w["V"] = noisy((num_users, k)), noisy((num_items, k))
    return w


def _ganmf_oracle(w, dtype):
    nu, k = w["U"].shape
    ni, e = w["We"].shape
    o = GANMFOracle(nu, ni, k, e, dtype=dtype)
    o.set_params(**w)
    return o


def _disganmf_oracle(w, act, dtype):
    nu, k = w["U"].shape
    ni = w["V"].shape[0]
    layers = sum(1 for n in w if n.startswith("W") and n[1:].isdigit())
    o = DisGANMFOracle(nu, ni, k, d_layers=layers, d_nodes=w["W0"].shape[1], d_hidden_act=act, dtype=dtype)
    o.set_params(**w)
    return o


def _inputs(o, urm, ids, generated):
    # (GANMFOracle.generator reads p["U"], p["V"] only: DisGANMFOracle, which has the same generator, borrows the line)
    return GANMFOracle.generator(o, ids) if generated else np.asarray(urm[ids].toarray(), dtype=o.dtype)


def _ganmf(w, urm, ids, generated, dtype):
    o = _ganmf_oracle(w, dtype)
    inp = _inputs(o, urm, ids, generated)
    E = inp @ o.p["We"] + o.p["be"]               # GANMFOracle.autoencoder's three lines, the mean taken per row
    R = E @ o.p["Wd"] + o.p["bd"]
    delta = R - inp
    energy = np.sum(delta * delta, axis=1) / o.dt(delta.shape[1])
    return E, energy


def _disganmf(w, act, urm, ids, generated, dtype, row_offset=0):
    o = _disganmf_oracle(w, act, dtype)
    _, feat, logit = o.discriminator(np.asarray(ids) + row_offset, _inputs(o, urm, ids, generated))
    return feat, logit


def oracle64(w, urm, ids, generated, act=None):
    """(features, value) in float64: GANMF (codes, per-row energies), or with `act` DisGANMF (last hidden features, logits)"""
    if act is None:
        return _ganmf(w, urm, ids, generated, np.float64)
    return _disganmf(w, act, urm, ids, generated, np.float64)


def restatement32(w, urm, ids, generated, act=None):
    """the same sequence in float32"""
    if act is None:
        return _ganmf(w, urm, ids, generated, np.float32)
    return _disganmf(w, act, urm, ids, generated, np.float32)


def deviations(got, ref64, relative):
    """the deviation the bound is about: largest absolute difference, or (energies) largest per-row relative one"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref64)
    return float((d / np.abs(ref64)).max()) if relative else float(d.max())


def floor_of(kind, num_items, ref64):
    """codes: sqrt(N) 2^-23 max|E|; energies (relative, per row): sqrt(N) 2^-23; logits and DisGANMF features: the codes' form with
    K = N + 2 input terms (profile, bias, uid) and the quantity's own largest magnitude"""
    if kind == "energy":
        return float(np.sqrt(num_items) * EPS32)
    big = float(np.abs(ref64).max()) if np.size(ref64) else 0.0
    K = num_items if kind == "codes" else num_items + 2
    return float(np.sqrt(K) * EPS32 * big)


def allowed(kind, num_items, ref64, ref32):
    """max(4 x the float32 restatement's own deviation from oracle64 on the same inputs, floor)"""
    return max(4.0 * deviations(ref32, ref64, kind == "energy"), floor_of(kind, num_items, ref64))


def ratio(kind, num_items, got, ref64, ref32):
    """deviation / allowed, and the two numbers"""
    dev, lim = deviations(got, ref64, kind == "energy"), allowed(kind, num_items, ref64, ref32)
    return dev / lim, dev, lim
