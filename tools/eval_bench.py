"""Hold-out evaluation wall time on ML-1M shapes: reference-order evaluator (all score rows to the host, per-user
python metrics) vs device top-k + block evaluator.  Usage: python tools/eval_bench.py

    python tools/eval_bench.py --candidates N

times instead the negative-sample protocol with N candidates per user (the test items included): ganmf_evaluate_candidates
(candidate scoring + top-k + metric sums, one call for all users) against the full-width ganmf_evaluate of the same users (user
blocks of 1e8 / n_items, as EvaluatorHoldoutFast calls it), alternating in one process, at two shapes with k = 250: ML-1M
(6040 x 3706) and the configs[3] shard width (25 000 x 50 000).  Host wall time around calls that end in a stream synchronise;
one JSON line per shape.

    python tools/eval_bench.py --groups 5

times ganmf_evaluate_groups with that many groups (users dealt to them at random), without and with the per-user values coming
back, beside ganmf_evaluate on the same handle and users, at the ML-1M shape (6040 x 3706, k = 250, cut-offs 5 / 10 / 20, one user
block): the three alternate in one process after a warm-up of each, host wall time around calls that end in a stream synchronise,
medians of `reps` calls in one JSON line; a second line gives the device time per kernel class of one profiled grouped call (a pass of
its own, after the timed ones).

    python tools/eval_bench.py --diversity

times EvaluatorHoldoutFast(test, [5, 10, 20], full_metrics=True, diversity_object=D).evaluateRecommender at the ML-1M shape (6040 x
3706, k = 250, random factors, D a random [3706, 3706] float32 matrix) through its device route (ganmf_evaluate_full +
ganmf_evaluate_diversity per user block) and through its host route (score matrix to the host, metrics and the list pairs in numpy),
alternating in one process after a warm-up of each, host wall time around calls that end in a stream synchronise, medians in one
JSON line; beside them the same evaluator without a diversity_object on the device route and the library call
ganmf_evaluate_diversity alone, for the cost of the extra call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganmf_amd.GANMF import GANMF  # noqa: E402
from ganmf_amd.evaluation import EvaluatorHoldout, EvaluatorHoldoutFast  # noqa: E402


def candidates_bench(n_candidates, cutoffs=(5, 10), reps=7):
    from ganmf_amd.engine import Engine
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    for name, (nu, ni) in (("ml1m", (6040, 3706)), ("configs3_shard", (25000, 50000))):
        rng = np.random.RandomState(0)
        k = 250
        eng = Engine(nu, ni, k, 16, 32)
        eng.set_tensor(100, rng.standard_normal((nu, k)).astype(np.float32))
        eng.set_tensor(101, rng.standard_normal((ni, k)).astype(np.float32))
        # per user: n_candidates distinct items, the first a test item (leave-one-out), 20 others seen
        cols = np.argsort(rng.rand(nu, 2 * n_candidates + 40), axis=1)[:, :n_candidates + 20] * (ni // (2 * n_candidates + 40))
        cols = (cols + rng.randint(0, ni // (2 * n_candidates + 40), size=cols.shape)).astype(np.int32)
        rows = np.repeat(np.arange(nu), n_candidates)
        cand = sps.csr_matrix((np.ones(nu * n_candidates, np.float32), (rows, cols[:, :n_candidates].ravel())), shape=(nu, ni))
        test = sps.csr_matrix((np.ones(nu, np.float32), (np.arange(nu), cols[:, 0])), shape=(nu, ni))
        seen = sps.csr_matrix((np.ones(nu * 20, np.float32), (np.repeat(np.arange(nu), 20), cols[:, n_candidates:].ravel())),
                              shape=(nu, ni))
        ev = EvaluatorHoldoutFast(test, list(cutoffs))
        eng.set_seen(seen)
        eng.set_test(ev._test_sorted, ev._test_gain)
        eng.set_candidates(cand)
        users = np.arange(nu)
        block = max(1, int(1e8 / ni))

        def full_width():
            out = None
            for lo in range(0, nu, block):
                part = eng.evaluate(users[lo:lo + block], cutoffs, ev._disc, ev._ideal_cum[lo:lo + block])
                out = part if out is None else out + part
            return out

        def candidates():
            return eng.evaluate_candidates(users, cutoffs, ev._disc, ev._ideal_cum)

        full_width(), candidates()                                   # warm-up: code objects, buffers, the split of V
        t_full, t_cand = [], []
        for _ in range(reps):                                        # alternating, every call ends in a stream synchronise
            t0 = time.perf_counter(); full_width(); t_full.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); candidates(); t_cand.append(time.perf_counter() - t0)
        f, c = float(np.median(t_full)) * 1e3, float(np.median(t_cand)) * 1e3
        print(json.dumps({"shape": name, "users": nu, "items": ni, "k": k, "candidates_per_user": n_candidates,
                          "cutoffs": list(cutoffs), "reps": reps, "full_width_evaluate_ms": round(f, 3),
                          "candidates_evaluate_ms": round(c, 3), "full_over_candidates": round(f / c, 2),
                          "full_width_ms_min_max": [round(min(t_full) * 1e3, 3), round(max(t_full) * 1e3, 3)],
                          "candidates_ms_min_max": [round(min(t_cand) * 1e3, 3), round(max(t_cand) * 1e3, 3)]}), flush=True)
        eng.close()


def groups_bench(n_groups, cutoffs=(5, 10, 20), reps=15):
    from ganmf_amd.engine import Engine
    from ganmf_amd.evaluation import EvaluatorHoldoutFast
    nu, ni, k = 6040, 3706, 250
    rng = np.random.RandomState(0)
    eng = Engine(nu, ni, k, 16, 32)
    eng.set_tensor(100, rng.standard_normal((nu, k)).astype(np.float32))
    eng.set_tensor(101, rng.standard_normal((ni, k)).astype(np.float32))
    seen = sps.random(nu, ni, density=0.04, format="csr", dtype=np.float32, random_state=1)
    test = sps.random(nu, ni, density=0.005, format="csr", dtype=np.float32, random_state=2)
    test.data[:] = rng.randint(1, 6, size=test.nnz)
    ev = EvaluatorHoldoutFast(test, list(cutoffs))
    eng.set_seen(seen)
    eng.set_test(ev._test_sorted, ev._test_gain)
    users = ev._users
    group_of = rng.randint(0, n_groups, size=len(users))
    calls = {"evaluate": lambda: eng.evaluate(users, cutoffs, ev._disc, ev._ideal_cum),
             "groups": lambda: eng.evaluate_groups(users, cutoffs, ev._disc, ev._ideal_cum, group_of, n_groups),
             "groups_per_user": lambda: eng.evaluate_groups(users, cutoffs, ev._disc, ev._ideal_cum, group_of, n_groups, per_user=True)}
    for fn in calls.values():                                        # warm-up: code objects, buffers, the split of V
        fn(), fn()
    times = {name: [] for name in calls}
    for _ in range(reps):                                            # alternating, every call ends in a stream synchronise
        for name, fn in calls.items():
            t0 = time.perf_counter(); fn(); times[name].append(time.perf_counter() - t0)
    med = {name: float(np.median(t)) * 1e3 for name, t in times.items()}
    sums, sizes, _ = calls["groups"]()
    assert np.allclose(sums.sum(axis=0), calls["evaluate"](), rtol=1e-12, atol=1e-9) and sizes.sum() == len(users)
    print(json.dumps({"shape": "ml1m", "users": int(len(users)), "items": ni, "k": k, "groups": n_groups, "cutoffs": list(cutoffs),
                      "reps": reps, "evaluate_ms": round(med["evaluate"], 3), "groups_ms": round(med["groups"], 3),
                      "groups_per_user_ms": round(med["groups_per_user"], 3),
                      "groups_over_evaluate": round(med["groups"] / med["evaluate"], 3),
                      "min_max_ms": {name: [round(min(t) * 1e3, 3), round(max(t) * 1e3, 3)] for name, t in times.items()}}), flush=True)
    eng.profile(True)
    calls["groups_per_user"]()
    print(json.dumps({"profiled_call": "groups_per_user", "device_ms_by_class": {p["name"]: round(p["ms"], 4) for p in eng.profile_read()}}),
          flush=True)
    eng.close()


def diversity_bench(cutoffs=(5, 10, 20), reps=9):
    nu, ni, k = 6040, 3706, 250
    rng = np.random.RandomState(0)
    train = sps.random(nu, ni, density=0.04, format="csr", dtype=np.float32, random_state=1)
    test = sps.random(nu, ni, density=0.005, format="csr", dtype=np.float32, random_state=2)
    test.data[:] = rng.randint(1, 6, size=test.nnz)
    model = GANMF(train, mode="user", is_experiment=True)
    model._build(k, 16, 32)
    model.engine.set_tensor(100, rng.standard_normal((nu, k)).astype(np.float32))
    model.engine.set_tensor(101, rng.standard_normal((ni, k)).astype(np.float32))
    model.URM_train = model._URM_eval
    D = rng.rand(ni, ni).astype(np.float32)
    dev_ev = EvaluatorHoldoutFast(test, list(cutoffs), full_metrics=True, diversity_object=D)
    host_ev = EvaluatorHoldoutFast(test, list(cutoffs), full_metrics=True, diversity_object=D)
    host_ev.use_device_metrics = False
    plain_ev = EvaluatorHoldoutFast(test, list(cutoffs), full_metrics=True)
    calls = {"device": lambda: dev_ev.evaluateRecommender(model)[0], "host": lambda: host_ev.evaluateRecommender(model)[0],
             "device_without_diversity": lambda: plain_ev.evaluateRecommender(model)[0]}
    rows = {name: fn() for name, fn in list(calls.items())}          # warm-up: code objects, buffers, uploads, the split of V
    for c in cutoffs:                                                # faster and different is not faster
        a, b = rows["device"][c]["DIVERSITY_SIMILARITY"], rows["host"][c]["DIVERSITY_SIMILARITY"]
        assert abs(a - b) <= 1e-12 * abs(b), (c, a, b)
        assert rows["device"][c]["MAP"] == rows["device_without_diversity"][c]["MAP"]
    # the library call alone, on the matrix the evaluator uploaded: ranking + list pairs + user sum, ending in a stream synchronise
    calls["evaluate_diversity_call"] = lambda: model.engine.evaluate_diversity(dev_ev._users, cutoffs)
    times = {name: [] for name in calls}
    for rep in range(reps):
        # the two device routes follow each other twice per repeat, taking turns to come first behind the (long) host route
        pair = ["device", "device_without_diversity"][::1 if rep % 2 == 0 else -1]
        for name in ["host"] + pair + pair + ["evaluate_diversity_call"] * 2:
            t0 = time.perf_counter(); calls[name](); times[name].append(time.perf_counter() - t0)
    med = {name: float(np.median(t)) * 1e3 for name, t in times.items()}
    print(json.dumps({"shape": "ml1m", "users": int(len(dev_ev._users)), "items": ni, "k": k, "cutoffs": list(cutoffs), "reps": reps,
                      "device_ms": round(med["device"], 3), "host_ms": round(med["host"], 3),
                      "device_without_diversity_ms": round(med["device_without_diversity"], 3),
                      "evaluate_diversity_call_ms": round(med["evaluate_diversity_call"], 3),
                      "host_over_device": round(med["host"] / med["device"], 2),
                      "min_max_ms": {name: [round(min(t) * 1e3, 3), round(max(t) * 1e3, 3)] for name, t in times.items()}}), flush=True)
    model.engine.close()


ap = argparse.ArgumentParser()
ap.add_argument("--candidates", type=int, default=0, help="N candidates per user (test items included): time the candidate route")
ap.add_argument("--groups", type=int, default=0, help="G groups: time ganmf_evaluate_groups beside ganmf_evaluate (ML-1M shape)")
ap.add_argument("--diversity", action="store_true", help="time the full row with a diversity_object: device route beside host route")
args = ap.parse_args()
if args.diversity:
    diversity_bench()
    sys.exit(0)
if args.groups:
    groups_bench(args.groups)
    sys.exit(0)
if args.candidates:
    candidates_bench(args.candidates)
    sys.exit(0)

g = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
train = sps.load_npz(os.path.join(g, "Movielens1M_URM_train.npz")).tocsr()
test = sps.load_npz(os.path.join(g, "Movielens1M_URM_test.npz")).tocsr()
model = GANMF(train, mode="user", is_experiment=True, seed=1)
model.fit(num_factors=250, emb_dim=992, epochs=1, batch_size=128, d_lr=1e-3, g_lr=1e-3, m=10, recon_coefficient=0.1)
slow_ev, fast_ev, host_ev = EvaluatorHoldout(test, [5]), EvaluatorHoldoutFast(test, [5]), EvaluatorHoldoutFast(test, [5])
host_ev.use_device_metrics = False      # device top-k ids, metrics in numpy on the host (round 1's fast evaluator)
# the 9-metric device route and the full 19-metric row (ganmf_evaluate_full) at the published cut-offs
acc4_ev = EvaluatorHoldoutFast(test, [5, 10, 20, 50])
full4_ev = EvaluatorHoldoutFast(test, [5, 10, 20, 50], full_metrics=True)
users = np.arange(train.shape[0])
for name, fn in (("slow evaluator", lambda: slow_ev.evaluateRecommender(model)),
                 ("fast evaluator, metrics on the host", lambda: host_ev.evaluateRecommender(model)),
                 ("fast evaluator, metrics on the device", lambda: fast_ev.evaluateRecommender(model)),
                 ("device, 9 metrics, cut-offs 5/10/20/50", lambda: acc4_ev.evaluateRecommender(model)),
                 ("device, full row, cut-offs 5/10/20/50", lambda: full4_ev.evaluateRecommender(model)),
                 ("device recommend top-5, all users", lambda: model.recommend_topk(users, 5)),
                 ("device recommend top-50, all users", lambda: model.recommend_topk(users, 50)),
                 ("host recommend top-5, all users", lambda: model.recommend(users, cutoff=5, return_scores=True))):
    fn()
    t0 = time.time()
    reps = 3 if name.startswith("slow") else 20
    for _ in range(reps):
        fn()
    print("%-40s %8.2f ms" % (name, (time.time() - t0) / reps * 1e3))
