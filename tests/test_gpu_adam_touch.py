"""Early touch of the Adam streams (csrc/adam_touch.hpp, GANMF_TUNE adam_touch): gV + Adam(V) on the fp32 ring kernel loads one dword of
every 128-byte line of its tile's theta / m / v in front of the K loop and never uses the values.  No arithmetic instruction changes, so
adam_touch=1 must reproduce adam_touch=0 BIT FOR BIT: every loss, all six parameter tensors, the Adam m and v slots.  The key is read
when a handle is created.  (That no touch leaves a tensor is shown on the CPU: tests/test_adam_touch_walk.py.)

The weight-gradient products of the discriminator step (gWd_ext, gWe_ext, DisGANMF's W_0) end in the same epilogue and do NOT touch: the
form that did was measured slower and left the library (profiles/r09_wgrad_touch.md); their cases stay, the key must be inert there."""
import numpy as np
import pytest

from ganmf_amd.synthetic import glorot_params, synthetic_urm

pytestmark = pytest.mark.gpu

IDS = {"We": 0, "be": 1, "Wd": 2, "bd": 3, "U": 100, "V": 101}
ADAM = tuple(IDS)      # every tensor's Adam slots (V carries the touch)
HP = dict(d_lr=1e-4, g_lr=2e-4, d_reg=1e-4, g_reg=0.0, m=10.0, recon_coefficient=0.05)

SHAPES = [
    (70, 65, 5, 33, 16),       # a second tile row of one row + the bias row; the last float4 straddles N (scalar tail, col + 3 >= N)
    (96, 129, 8, 64, 32),      # e is exactly one tile; N + 1 is two tiles plus two rows
    (64, 63, 4, 7, 32),        # a single partial tile for both products
    # ... and two for the edges of V [N, k] itself (gUb + gV ride in pair_kernel, whose gV range carries the touch) with longer K ranges:
    (200, 65, 5, 33, 96),      # V [65, 5]: a second tile row of one row, the float4 at column 4 straddles k; ragged last batch (K = 8)
    (150, 129, 70, 64, 80),    # V [129, 70]: two tile columns, the second partial with a straddling float4 (68 .. 71), three tile rows
]


def _run(monkeypatch, touch, U, N, k, e, B, tune=""):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    monkeypatch.setenv("GANMF_TUNE", tune + "adam_touch=%d" % touch)
    urm = synthetic_urm(U, N, 0.04, seed=21)
    w = glorot_params(U, N, k, e, seed=9)
    eng = Engine(U, N, k, e, B, **HP)
    eng.set_urm(urm)
    for n, tid in IDS.items():
        eng.set_tensor(tid, w[n])
    rng = np.random.RandomState(5)
    losses = []
    for _ in range(2):
        dl, gl = eng.train_epoch(rng.permutation(U), 1, 1)
        losses.append((np.array(dl), np.array(gl)))
    out = {n: eng.get_tensor(tid).copy() for n, tid in IDS.items()}
    out.update({n + ".m": eng.get_tensor(IDS[n], slot=L.SLOT_ADAM_M).copy() for n in ADAM})
    out.update({n + ".v": eng.get_tensor(IDS[n], slot=L.SLOT_ADAM_V).copy() for n in ADAM})
    eng.close()
    return out, losses


def _same(got, ref, what):
    (g, gl), (r, rl) = got, ref
    assert len(gl) == len(rl)
    for (dl, gg), (dr, gr) in zip(gl, rl):
        np.testing.assert_array_equal(dl, dr, err_msg="D losses, " + what)
        np.testing.assert_array_equal(gg, gr, err_msg="G losses, " + what)
    assert set(g) == set(r)
    for n in r:
        np.testing.assert_array_equal(g[n], r[n], err_msg="%s, %s" % (n, what))


@pytest.mark.parametrize("shape", SHAPES)
def test_adam_touch_bit_identical(shape, monkeypatch):
    ref = _run(monkeypatch, 0, *shape)
    got = _run(monkeypatch, 1, *shape)
    _same(got, ref, "adam_touch=1 vs 0 at %r" % (shape,))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_adam_touch_bit_identical_four_wave_pair(shape, monkeypatch):
    """The touch on 256-thread workgroups, where a thread touches up to two lines: gUb and gV as separate launches (GANMF_MULTI bit 1 clear)
    on a one-K-group plan (GANMF_TUNE kg=1), so gV + Adam(V) runs gemm_f32_mfma<64, 64, 64, 2, true, true, 1> (GANMF_DEBUG_PLAN=1 prints
    "kg 1" for gemm_gV at both shapes)."""
    monkeypatch.setenv("GANMF_MULTI", str(127 & ~2))
    ref = _run(monkeypatch, 0, *shape, tune="kg=1,")
    got = _run(monkeypatch, 1, *shape, tune="kg=1,")
    _same(got, ref, "separate gV launch, kg=1, adam_touch=1 vs 0 at %r" % (shape,))


def test_adam_touch_inert_under_forced_collectives(monkeypatch):
    """The data-parallel discriminator step does not fuse Adam into its weight-gradient products: the key must change nothing there."""
    monkeypatch.setenv("GANMF_FORCE_COLLECTIVES", "1")
    shape = SHAPES[0]
    ref = _run(monkeypatch, 0, *shape)
    got = _run(monkeypatch, 1, *shape)
    _same(got, ref, "GANMF_FORCE_COLLECTIVES=1, adam_touch=1 vs 0")


def _run_dis(monkeypatch, touch, U, N, k, e, B, layers):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    monkeypatch.setenv("GANMF_TUNE", "adam_touch=%d" % touch)
    rng = np.random.RandomState(17)
    urm = synthetic_urm(U, N, 0.06, seed=4)
    ids = {}
    for l in range(layers):
        ids["W%d" % l], ids["b%d" % l] = 2 * l, 2 * l + 1
    ids["Wo"], ids["bo"], ids["U"], ids["V"] = 2 * layers, 2 * layers + 1, 100, 101
    eng = Engine(U, N, k, e, B, model=L.MODEL_DISGANMF, d_layers=layers, d_act="tanh", d_lr=1e-3, g_lr=2e-3, d_reg=1e-4, g_reg=0.0,
                 m=0.0, recon_coefficient=0.3)
    eng.set_urm(urm)
    for n, tid in ids.items():
        r, c = eng.shape(tid)
        a = (rng.randn(r, c) * 0.05).astype(np.float32)
        if n == "W0":
            a[0, :] *= 1.0 / U      # the float(uid) row: keep tanh off its flat ends
        eng.set_tensor(tid, a)
    prng = np.random.RandomState(5)
    losses = []
    for _ in range(2):
        dl, gl = eng.train_epoch(prng.permutation(U), 1, 1)
        losses.append((np.array(dl), np.array(gl)))
    out = {n: eng.get_tensor(tid).copy() for n, tid in ids.items()}
    for n, tid in ids.items():
        if n not in ("U", "V"):
            out[n + ".m"] = eng.get_tensor(tid, slot=L.SLOT_ADAM_M).copy()
            out[n + ".v"] = eng.get_tensor(tid, slot=L.SLOT_ADAM_V).copy()
    eng.close()
    return out, losses


def test_adam_touch_bit_identical_disganmf(monkeypatch):
    """DisGANMF's W_0 gradient ([X;F | 1 | uid]^T . dz_0, N + 2 rows) ends in the same epilogue."""
    shape = (70, 65, 5, 33, 16)
    ref = _run_dis(monkeypatch, 0, *shape, layers=1)
    got = _run_dis(monkeypatch, 1, *shape, layers=1)
    _same(got, ref, "DisGANMF, adam_touch=1 vs 0")
