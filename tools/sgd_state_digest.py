#!/usr/bin/env python3
"""Digests of everything the SGD trainers write (SLIM-BPR, MF-BPR, FunkSVD), for comparing two builds of the library byte for byte.

  GANMF_LIB_PATH=/path/to/one/libganmf_hip.so   python tools/sgd_state_digest.py --out a.json
  GANMF_LIB_PATH=/path/to/other/libganmf_hip.so python tools/sgd_state_digest.py --out b.json      # a fresh process each
  python tools/sgd_state_digest.py --compare a.json b.json                                            # needs no GPU

Every configuration draws seeded samples (*_draw), trains three epochs (*_epochs) and prints the sha256 of the drawn arrays, of every
block of *_get_state, of the beta powers and of n_levels; SLIM-BPR also of the CSR left by ganmf_slim_bpr_finish.
  SLIM-BPR: the 40 x 70 and 40 x 400 profiles of tests/test_gpu_slim_bpr.py; {dense, symmetric} x the four sgd modes x the routes the
            storage allows (dense: sequential and levelled; symmetric: sequential).
  MF:       the 70 x 50 profiles of tests/test_gpu_mf_sgd.py at num_factors 1 and 65; {MF_BPR, FUNK_SVD, FUNK_SVD with biases} x the
            four modes x both routes, FunkSVD at negative_interactions_quota 0 and 0.3; batch_size 16.
A few seconds on one GPU.  A run without a GPU fails: there is no fallback."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ["sgd", "adagrad", "rmsprop", "adam"]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def slim_digests(out):
    from ganmf_amd import _lib as L
    from ganmf_amd.engine import Engine
    from tests import test_gpu_slim_bpr as T
    for n_items in (70, 400):
        urm = sps.csr_matrix(T._urm(n_items), dtype=np.float32)
        urm.sort_indices()
        for symmetric in (False, True):
            routes = [("sequential", L.SLIM_SEQUENTIAL)] + ([] if symmetric else [("levelled", L.SLIM_LEVELLED)])
            for mode in MODES:
                for route_name, route in routes:
                    label = "slim items=%d %s %s %s" % (n_items, "symmetric" if symmetric else "dense", mode, route_name)
                    eng = Engine(40, n_items, 1, 1, 1, model=L.MODEL_ITEMSIM)
                    eng.slim_bpr_init(symmetric=symmetric, sgd_mode=mode, seed=5, profiles=urm, **T.HP)
                    out[label + " | draw"] = sha(*eng.slim_bpr_draw(0, 2))
                    levels = eng.slim_bpr_epochs(3, mode=route)
                    state = eng.slim_bpr_state()
                    for name in ("S", "state0", "state1", "beta_powers"):
                        out[label + " | " + name] = sha(state[name])
                    out[label + " | n_levels, epoch"] = sha(np.array([levels, state["epoch"]], dtype=np.int64))
                    eng.slim_bpr_finish(10)
                    W = eng.item_similarity().tocsr()
                    out[label + " | finish CSR"] = sha(W.indptr.astype(np.int64), W.indices.astype(np.int32), W.data.astype(np.float32))
                    eng.close()


def mf_digests(out):
    from ganmf_amd import _lib as L
    from tests import helpers_mf_sgd as H
    from tests import test_gpu_mf_sgd as T
    urm = T._urm()
    for k in (1, 65):
        U0, V0 = T._factors(urm, k)
        for algorithm, use_bias in T.CONFIGS:
            for quota in ((0.0,) if algorithm == "MF_BPR" else (0.0, 0.3)):
                for mode in MODES:
                    for route_name, route in (("sequential", L.MF_SGD_SEQUENTIAL), ("levelled", L.MF_SGD_LEVELLED)):
                        label = "mf k=%d %s bias=%d quota=%.1f %s %s" % (k, algorithm, use_bias, quota, mode, route_name)
                        eng = T._engine(urm, algorithm, use_bias, mode, U0, V0, seed=5, quota=quota)
                        out[label + " | draw"] = sha(*eng.mf_sgd_draw(0, 1, batch_size=16))
                        levels = eng.mf_sgd_epochs(3, batch_size=16, route=route)
                        state = eng.mf_sgd_state()
                        for block in ("params", "state0", "state1"):
                            out[label + " | " + block] = sha(*[state[block][n] for n in H.MEMBERS])
                        out[label + " | beta_powers"] = sha(state["beta_powers"])
                        out[label + " | n_levels, epoch"] = sha(np.array([levels, state["epoch"]], dtype=np.int64))
                        eng.close()


def compare(path_a, path_b):
    a, b = json.load(open(path_a)), json.load(open(path_b))
    keys = sorted(set(a) | set(b))
    differing = [k for k in keys if a.get(k) != b.get(k)]
    for k in differing:
        print("DIFFERS  %s: %s | %s" % (k, a.get(k), b.get(k)))
    groups = {}
    for k in keys:
        g = k.split(" ")[0] + " | " + k.split(" | ")[1]
        same, n = groups.get(g, (0, 0))
        groups[g] = (same + (a.get(k) == b.get(k)), n + 1)
    for g in sorted(groups):
        print("%-28s %3d of %3d digests equal" % (g, groups[g][0], groups[g][1]))
    print("%d digests, %d differ" % (len(keys), len(differing)))
    return 1 if differing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    out = {}
    slim_digests(out)
    mf_digests(out)
    for k in sorted(out):
        print("%s  %s" % (out[k][:16], k))
    print("%d digests; all of them: %s" % (len(out), hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
