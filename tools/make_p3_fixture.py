#!/usr/bin/env python3
"""Writes the two P3alpha / RP3beta fixtures of the suite from the reference implementation, which is imported from the path given
on the command line (nothing of it is copied):

  tests/golden/p3_tiny.npz             a 40 x 30 matrix with integer ratings 1..5 (the recipe of make_itemknn_fixture.tiny_matrix
                                       with another seed) and, per case, the dense W_sparse that the reference's P3alphaRecommender
                                       or RP3betaRecommender returns for it.  Every case is asserted TIE-FREE: the float64
                                       restatement (tests/helpers_p3.py) selects the same pattern under "smaller id" and under
                                       "larger id", so the reference's arbitrary tie order cannot matter.
  tests/golden/p3_trial_logs_ml1m.json the first three logged trials of experiments/P3alphaRecommender__1M/results.txt plus the
                                       best_params.txt row, each with MAP@5 four times: `logged`, `replayed` (the reference class
                                       fitted on tests/golden/Movielens1M_URM_train_small.npz, evaluated on
                                       Movielens1M_URM_validation.npz), `restated64` and `restated32` (the restatement, and the
                                       restatement with the product taken in float32, through the same evaluator), and `latitude`:
                                       the largest distance of the other three from `replayed`.

usage: make_p3_fixture.py /path/to/reference [--tiny-only] [--trials-only]
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_USERS_ML1M = 6040

# (the seeds 20240 and 20242 each give one case with an exact tie at a cut; 20241 gives none)
TINY_SEED = 20241
TINY_CASES = [
    dict(model="P3alpha", topK=5, alpha=0.7, normalize_similarity=True),
    dict(model="P3alpha", topK=3, alpha=1.0),
    dict(model="P3alpha", topK=29, alpha=1.6, normalize_similarity=True),
    dict(model="P3alpha", topK=100, alpha=0.3),
    # implicit data are ones, so the walk's values repeat: at topK = 5 (and at every topK below 24) some row or column has an exact tie
    # at its cut; 24 is the smallest tie-free topK, and it still cuts (446 of the 452 non-zero entries survive)
    dict(model="P3alpha", topK=24, alpha=0.7, min_rating=3, implicit=True),
    dict(model="RP3beta", topK=6, alpha=0.8, beta=0.4, normalize_similarity=True),
    dict(model="RP3beta", topK=4, alpha=1.0, beta=1.2, normalize_similarity=False),
]


def tiny_matrix():
    rng = np.random.RandomState(TINY_SEED)
    m = (rng.rand(40, 30) < 0.25) * rng.randint(1, 6, (40, 30))
    m[:, 11] = 0      # an item nobody rated
    m[7, :] = 0       # a user without ratings
    return sps.csr_matrix(m.astype(np.float32))


def reference_class(model):
    if model == "P3alpha":
        from GraphBased.P3alphaRecommender import P3alphaRecommender
        return P3alphaRecommender
    from GraphBased.RP3betaRecommender import RP3betaRecommender
    return RP3betaRecommender


def restated(H, urm, case, **kw):
    data = H.apply_min_rating(urm, case.get("min_rating", 0), case.get("implicit", False))
    return H.fit(data, topK=case["topK"], alpha=case["alpha"], beta=case.get("beta"),
                 normalize_similarity=case.get("normalize_similarity", False), **kw)


def make_tiny(H, out_path):
    urm = tiny_matrix()
    arrays = {"urm": np.asarray(urm.todense(), dtype=np.float32), "cases": np.array(json.dumps(TINY_CASES))}
    for n, case in enumerate(TINY_CASES):
        a, b = restated(H, urm, case), restated(H, urm, case, larger_id=True)
        if (a != b).nnz != 0:
            raise SystemExit("case %d %r has an exact tie at a cut: the two tie rules select different patterns; change its topK "
                             "or the seed" % (n, case))
        args = dict(case)
        rec = reference_class(args.pop("model"))(urm.copy())
        rec.fit(**args)
        W = np.asarray(rec.W_sparse.todense(), dtype=np.float64)
        assert ((W != 0) == (a.toarray() != 0)).all(), "case %d: the reference's pattern is not the restatement's" % n
        np.testing.assert_allclose(a.toarray(), W, rtol=1e-6, atol=0)
        arrays["W_%d" % n] = W
        print("case", n, case, "nnz", int((W != 0).sum()), flush=True)
    np.savez_compressed(out_path, **arrays)
    print("wrote", out_path)


def logged_trials(reference):
    """[(params, MAP@5)] of results.txt in file order"""
    text = open(os.path.join(reference, "experiments", "P3alphaRecommender__1M", "results.txt")).read()
    out = []
    for m in re.finditer(r"(\{[^\n]*\})\nCUTOFF: 5 - [^\n]*?MAP: ([0-9.]+),", text):
        out.append((json.loads(m.group(1)), float(m.group(2))))
    return out


def map_at_5(rec, valid):
    from Base.Evaluation.Evaluator import EvaluatorHoldout
    results, _ = EvaluatorHoldout(valid, cutoff_list=[5]).evaluateRecommender(rec)
    return float(results[5]["MAP"])


def make_trials(H, reference, out_path):
    from GraphBased.P3alphaRecommender import P3alphaRecommender
    train = sps.load_npz(os.path.join(GOLDEN, "Movielens1M_URM_train_small.npz")).tocsr()
    valid = sps.load_npz(os.path.join(GOLDEN, "Movielens1M_URM_validation.npz")).tocsr()
    assert train.shape[0] == N_USERS_ML1M
    logged = logged_trials(reference)
    best = json.load(open(os.path.join(reference, "experiments", "P3alphaRecommender__1M", "best_params.txt")))
    best_logged = [v for p, v in logged if p == best]
    rows = [("trial", p, v) for p, v in logged[:3]] + [("best", best, best_logged[0] if best_logged else None)]
    trials, latitude = [], 0.0
    for role, params, value in rows:
        rec = P3alphaRecommender(train.copy())
        rec.fit(**params)
        replayed = map_at_5(rec, valid)
        case = dict(params)
        holder = P3alphaRecommender(train.copy())      # the reference's scoring and evaluator around the restatement's W
        holder.W_sparse = sps.csr_matrix(restated(H, train, case))
        restated64 = map_at_5(holder, valid)
        holder.W_sparse = sps.csr_matrix(restated(H, train, case, dtype=np.float32))
        restated32 = map_at_5(holder, valid)
        others = [restated64, restated32] + ([value] if value is not None else [])
        latitude = max([latitude] + [abs(v - replayed) for v in others])
        trials.append(dict(role=role, params=params, logged=value, replayed=replayed, restated64=restated64, restated32=restated32))
        print(role, params, "logged", value, "replayed", replayed, "restated64", restated64, "restated32", restated32, flush=True)
    # the suite's bound on the device, 4 * latitude + 1e-6, must stay below the step of MAP@5 when ONE user's list goes wrong
    assert 4 * latitude + 1e-6 < 1.0 / (2 * N_USERS_ML1M), latitude
    doc = dict(source="experiments/P3alphaRecommender__1M/results.txt and best_params.txt of the reference",
               metric="MAP", at=5, train="Movielens1M_URM_train_small.npz", validation="Movielens1M_URM_validation.npz",
               latitude=latitude, trials=trials)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path, "latitude", latitude)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--tiny-only", action="store_true")
    ap.add_argument("--trials-only", action="store_true")
    a = ap.parse_args()
    # tests.helpers_p3 of this repository first, then the repository leaves the path again: the reference's GraphBased/ has no
    # __init__.py, and this repository's package of the same name would be preferred to it wherever it stands on the path
    sys.path.insert(0, ROOT)
    from tests import helpers_p3 as H
    sys.path.remove(ROOT)
    assert "GraphBased" not in sys.modules
    sys.path.insert(0, os.path.abspath(a.reference))
    for name, kind in (("int", int), ("float", float), ("bool", bool), ("object", object)):
        if name not in np.__dict__:      # aliases the reference still uses, removed in numpy 1.24
            setattr(np, name, kind)
    if not a.trials_only:
        make_tiny(H, os.path.join(GOLDEN, "p3_tiny.npz"))
    if not a.tiny_only:
        make_trials(H, os.path.abspath(a.reference), os.path.join(GOLDEN, "p3_trial_logs_ml1m.json"))


if __name__ == "__main__":
    main()
