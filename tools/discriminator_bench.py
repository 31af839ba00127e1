"""Discriminator inference (ganmf_discriminate) wall time at the ML-1M shape: 6040 rows x 3706 items, k = 250, emb_dim = 992, all
rows, codes + energies, for the stored and for the generated profiles.  Usage: python tools/discriminator_bench.py [--reps 7]

Times, alternating in one process (median of --reps repeats, host wall time around calls that end in a stream synchronise):

  * the device call: codes + energies of all stored rows, codes + energies of all generated rows, and each output alone;
  * the host route of the code before this entry existed, on the same box:
      codes     autoencoder_codes() as it was: the encoder fetched from the device, URM_train . We + be as a scipy product;
      energies  the rows on the host (URM_train.toarray(), or the scores fetched through ganmf_scores for generated rows), then the
                reference's float32 sequence in numpy -- E = x We + be, R = E Wd + bd, mean_j (R - x)^2 -- on the BLAS threads the
                environment gives (OMP_NUM_THREADS; 16 on the measurement boxes), weights fetched once outside the timed part.

and reads the energy launch's device time from the library's profile (ganmf_profile_read) for its achieved TFLOP/s against the fp32
MFMA roof (the launch is compute-bound: 2 n N (e + 1) FLOP over at most 4 (n (e + 1) + (e + 1) N + n N) operand bytes).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_ROOF_TFLOPS = 157.3      # MI355X, dense fp32 matrix peak

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rows", type=int, default=6040)
ap.add_argument("--items", type=int, default=3706)
ap.add_argument("--factors", type=int, default=250)
ap.add_argument("--emb-dim", type=int, default=992)
args = ap.parse_args()

NU, NI, K, E = args.rows, args.items, args.factors, args.emb_dim
rng = np.random.RandomState(0)
glorot = lambda a, b: rng.uniform(-np.sqrt(6.0 / (a + b)), np.sqrt(6.0 / (a + b)), size=(a, b)).astype(np.float32)
w = {0: glorot(NI, E), 1: (0.05 * rng.randn(E)).astype(np.float32), 2: glorot(E, NI), 3: (0.05 * rng.randn(NI)).astype(np.float32),
     100: glorot(NU, K), 101: glorot(NI, K)}
urm = sps.random(NU, NI, density=0.045, format="csr", dtype=np.float32, random_state=rng)      # ML-1M's density
urm.data[:] = 1.0
rows = np.arange(NU, dtype=np.int32)

from ganmf_amd.engine import Engine      # noqa: E402

eng = Engine(NU, NI, K, E, 64)
eng.set_urm(urm)
for tid, a in w.items():
    eng.set_tensor(tid, a)


def host_codes():
    We, be = eng.get_tensor(0), eng.get_tensor(1)[0]
    return np.asarray(urm.dot(We) + be, dtype=np.float32)


WE, BE, WD, BD = w[0], w[1], w[2], w[3]


def host_energy(generated):
    x = eng.scores(rows) if generated else np.asarray(urm.toarray(), dtype=np.float32)
    code = x @ WE + BE
    delta = code @ WD + BD
    delta -= x
    return np.einsum("ij,ij->i", delta, delta) / np.float32(NI)


def median_ms(fns, reps):
    times = {name: [] for name, _ in fns}
    for name, fn in fns:
        fn()                                              # warm-up: code objects, buffers
    for _ in range(reps):                                 # alternating
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)) for name, t in times.items()}


fns = [("device_stored_codes_energies", lambda: eng.discriminate(rows)),
       ("device_generated_codes_energies", lambda: eng.discriminate(rows, generated=True)),
       ("device_stored_codes", lambda: eng.discriminate(rows, value=False)),
       ("device_stored_energies", lambda: eng.discriminate(rows, features=False)),
       ("device_generated_energies", lambda: eng.discriminate(rows, generated=True, features=False)),
       ("host_stored_codes", host_codes),
       ("host_stored_energies", lambda: host_energy(False)),
       ("host_generated_energies", lambda: host_energy(True))]
res = median_ms(fns, args.reps)

out = {"shape": "ml1m" if (NU, NI, K, E) == (6040, 3706, 250, 992) else "custom", "rows": NU, "items": NI, "k": K, "emb_dim": E,
       "reps": args.reps, "host_blas_threads": os.environ.get("OMP_NUM_THREADS"), "fp32_mfma_roof_tflops": FP32_MFMA_ROOF_TFLOPS}
for name, (med, lo, hi) in res.items():
    out[name + "_ms"] = med
    out[name + "_ms_min_max"] = [lo, hi]
out["host_over_device_stored_codes"] = round(res["host_stored_codes"][0] / res["device_stored_codes"][0], 1)
out["host_over_device_stored_energies"] = round(res["host_stored_energies"][0] / res["device_stored_energies"][0], 1)
out["host_over_device_generated_energies"] = round(res["host_generated_energies"][0] / res["device_generated_energies"][0], 1)
# agreement of the two routes (float32 host sequence against the device), for the record
dev_c, dev_v = eng.discriminate(rows)
out["codes_max_abs_diff_host_device"] = float(np.abs(dev_c - host_codes()).max())
out["energies_max_rel_diff_host_device"] = float(np.abs(dev_v / host_energy(False).astype(np.float64) - 1.0).max())
for generated in (False, True):
    eng.profile(True)
    for _ in range(5):
        eng.discriminate(rows, generated=generated, features=False)
    prof = {e["name"]: e for e in eng.profile_read()}
    eng.profile(False)
    dec = [e for name, e in prof.items() if name.startswith("gemm_decode")][0]
    ms = dec["ms"] / dec["launches"]
    key = "generated" if generated else "stored"
    out["energy_launch_%s_ms" % key] = round(ms, 4)
    out["energy_launch_%s_tflops" % key] = round(dec["flops"] / dec["launches"] / ms * 1e-9, 1)
    out["energy_launch_%s_fraction_of_fp32_mfma_roof" % key] = round(dec["flops"] / dec["launches"] / ms * 1e-9 / FP32_MFMA_ROOF_TFLOPS, 3)
print(json.dumps(out), flush=True)
eng.close()
