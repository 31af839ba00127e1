#!/usr/bin/env python3
"""Writes tests/golden/mf_sgd_tiny.npz: what the reference's compiled SGD epoch computes on a 40 x 30 matrix, as data.

    python tools/make_mf_sgd_fixture.py --reference /path/to/the/reference/tree

The reference ships MatrixFactorization/Cython/MatrixFactorization_Cython_Epoch.pyx with a binary for CPython 3.6 only.  This tool
compiles the .pyx with the Cython that is installed into a temporary directory (nothing of it is kept), runs the epoch object with
random_seed set -- which seeds C rand() -- with batch_size 8 for 3 epochs per case, and records per case the parameters, the initial
and final factors and biases and the sample list that tests/helpers_mf_sgd.py's restatement of glibc's rand() predicts for that seed.
It refuses to write unless the float64 restatement (R_seq) applied to the predicted list from the recorded initial factors reproduces
the reference's final state to 1e-12 relative: that proves the restatement and the emulated stream together.

Cases: MF_BPR with the four sgd modes; FUNK_SVD with use_bias on / off x negative_interactions_quota 0 / 0.3 x sgd / adam, each with
the arguments the reference's own fit() forwards to the epoch object."""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import helpers_mf_sgd as H  # noqa: E402

N_USERS, N_ITEMS, BATCH, EPOCHS, FACTORS = 40, 30, 8, 3, 6
RATES = dict(learning_rate=0.05, user_reg=0.01, item_reg=0.04, bias_reg=0.003, positive_reg=0.02, negative_reg=0.005)


def matrix():
    rng = np.random.RandomState(7)
    m = (rng.rand(N_USERS, N_ITEMS) < 0.2) * rng.randint(1, 6, size=(N_USERS, N_ITEMS))
    m[3] = 0                                        # never drawn: empty
    m[11] = rng.randint(1, 6, size=N_ITEMS)         # never drawn: full
    m[17] = 0
    m[17, 4] = 5                                    # a single positive
    return sps.csr_matrix(m.astype(np.float64))


def cases():
    out = []
    for k, mode in enumerate(H.MODES):
        out.append(dict(algorithm="MF_BPR", sgd_mode=mode, use_bias=False, quota=0.0, seed=100 + k))
    k = 0
    for use_bias in (True, False):
        for quota in (0.0, 0.3):
            for mode in ("sgd", "adam"):
                out.append(dict(algorithm="FUNK_SVD", sgd_mode=mode, use_bias=use_bias, quota=quota, seed=200 + k))
                k += 1
    return out


def build_epoch_module(reference, scratch):
    """the reference's .pyx compiled in `scratch`; returns the module"""
    from Cython.Build import cythonize
    from setuptools import Extension
    from setuptools.dist import Distribution
    name = "MatrixFactorization_Cython_Epoch"
    src = os.path.join(scratch, name + ".pyx")
    shutil.copy(os.path.join(reference, "MatrixFactorization", "Cython", name + ".pyx"), src)
    directives = dict(language_level=3, boundscheck=False, wraparound=False, initializedcheck=False, nonecheck=False, cdivision=True,
                      overflowcheck=False)
    ext = cythonize([Extension(name, [src], include_dirs=[np.get_include()], extra_compile_args=["-O2", "-ffp-contract=off"])],
                    compiler_directives=directives, build_dir=scratch, quiet=True)
    dist = Distribution({"ext_modules": ext, "script_name": "build", "script_args": []})
    cmd = dist.get_command_obj("build_ext")
    cmd.build_lib = scratch
    cmd.build_temp = os.path.join(scratch, "obj")
    cmd.ensure_finalized()
    cmd.run()
    sys.path.insert(0, scratch)
    return importlib.import_module(name)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds Base/ and MatrixFactorization/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mf_sgd_tiny.npz"))
    args = ap.parse_args()
    for alias, kind in (("int", int), ("float", float), ("bool", bool)):      # aliases numpy removed, which the .pyx still names
        if not hasattr(np, alias):
            setattr(np, alias, kind)
    sys.path.append(os.path.abspath(args.reference))      # Base.Recommender_utils.check_matrix, imported by the .pyx
    scratch = tempfile.mkdtemp(prefix="mf_sgd_fixture_")
    try:
        module = build_epoch_module(os.path.abspath(args.reference), scratch)
        urm = matrix()
        out = {"urm_data": urm.data, "urm_indices": urm.indices.astype(np.int32), "urm_indptr": urm.indptr.astype(np.int64),
               "urm_shape": np.array(urm.shape, dtype=np.int64), "batch_size": np.array(BATCH), "epochs": np.array(EPOCHS)}
        worst = 0.0
        for n, case in enumerate(cases()):
            bpr = case["algorithm"] == "MF_BPR"
            kw = dict(algorithm_name=case["algorithm"], n_factors=FACTORS, learning_rate=RATES["learning_rate"], sgd_mode=case["sgd_mode"],
                      user_reg=RATES["user_reg"], batch_size=BATCH, use_bias=case["use_bias"], init_mean=0.0, init_std_dev=0.1,
                      verbose=False, random_seed=case["seed"])
            if bpr:      # MatrixFactorization_Cython.py:91-104
                kw.update(positive_reg=RATES["positive_reg"], negative_reg=RATES["negative_reg"])
            else:        # :64-78
                kw.update(item_reg=RATES["item_reg"], bias_reg=RATES["bias_reg"], negative_interactions_quota=case["quota"])
            epoch = module.MatrixFactorization_Cython_Epoch(urm.copy(), **kw)
            U0, V0 = epoch.get_USER_factors().copy(), epoch.get_ITEM_factors().copy()
            for _ in range(EPOCHS):
                epoch.epochIteration_Cython()
            final = {"USER_factors": epoch.get_USER_factors(), "ITEM_factors": epoch.get_ITEM_factors()}
            if case["use_bias"]:
                final.update(USER_bias=epoch.get_USER_bias(), ITEM_bias=epoch.get_ITEM_bias(),
                             GLOBAL_bias=np.array([float(epoch.get_GLOBAL_bias())]))
            total = EPOCHS * H.per_epoch(case["algorithm"], urm, BATCH)
            samples = H.reference_samples(case["algorithm"], H.GlibcRand(case["seed"]), total, urm, case["quota"])
            rates = dict(learning_rate=H.f32(RATES["learning_rate"]), user_reg=H.f32(RATES["user_reg"]))
            if bpr:
                rates.update(positive_reg=H.f32(RATES["positive_reg"]), negative_reg=H.f32(RATES["negative_reg"]))
            else:
                rates.update(bias_reg=H.f32(RATES["bias_reg"]))
            got = H.Trainer(case["algorithm"], U0, V0, case["use_bias"], case["sgd_mode"], **rates).apply(*samples, batch_size=BATCH).params()
            for name, ref in final.items():
                err = float(np.abs(got[name] - ref).max() / np.abs(ref).max())
                worst = max(worst, err)
                if not err <= 1e-12:
                    raise SystemExit("case %d %r: %s of the restatement differs from the reference by %.3e relative: nothing written"
                                     % (n, case, name, err))
            moved = float(np.abs(final["USER_factors"] - U0).max())
            print("case %2d %-8s %-7s bias %-5s quota %.1f: %d samples, max |U - U0| %.3e, restatement within %.1e" % (
                n, case["algorithm"], case["sgd_mode"], case["use_bias"], case["quota"], total, moved, worst))
            params = dict(case, num_factors=FACTORS, **RATES)
            out["c%d_params" % n] = np.array(json.dumps(params, sort_keys=True))
            out["c%d_U0" % n], out["c%d_V0" % n] = U0, V0
            out["c%d_users" % n], out["c%d_items" % n], out["c%d_third" % n] = samples
            for name, ref in final.items():
                out["c%d_%s" % (n, name)] = np.asarray(ref, dtype=np.float64)
        out["n_cases"] = np.array(len(cases()))
        np.savez_compressed(args.out, **out)
        print("wrote %s (%d bytes); worst relative difference %.2e" % (args.out, os.path.getsize(args.out), worst))
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
