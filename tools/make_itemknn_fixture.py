#!/usr/bin/env python3
"""Writes the two item-KNN fixtures of the suite from the reference implementation, which is imported from the path given on the
command line (nothing of it is copied):

  tests/golden/itemknn_tiny.npz             a 40 x 30 matrix with integer ratings 1..5 and, per case, the dense W_sparse that the
                                            reference's Compute_Similarity_Python returns for it (every similarity kind with a few
                                            (topK, shrink, normalize, alpha, beta) settings, and both feature weightings)
  tests/golden/itemknn_trial_logs_ml1m.json the first three logged trials of each similarity kind from
                                            experiments/ItemKNNCFRecommender_<kind>_1M/results.txt plus the best_params.txt row, each
                                            with the logged MAP@5 and `replayed`: the MAP@5 of the reference's Python class fitted on
                                            tests/golden/Movielens1M_URM_train_small.npz and evaluated on Movielens1M_URM_validation.npz

usage: make_itemknn_fixture.py /path/to/reference [--tiny-only] [--trials-only]
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
KINDS = ["cosine", "asymmetric", "jaccard", "dice", "tversky"]

TINY_CASES = [
    dict(similarity="cosine", topK=5, shrink=0, normalize=True),
    dict(similarity="cosine", topK=29, shrink=10, normalize=True),
    dict(similarity="cosine", topK=7, shrink=3, normalize=False),
    dict(similarity="cosine", topK=7, shrink=0, normalize=False),
    dict(similarity="asymmetric", topK=6, shrink=2, normalize=True, asymmetric_alpha=0.25),
    dict(similarity="asymmetric", topK=100, shrink=0, normalize=True, asymmetric_alpha=0.8),
    dict(similarity="jaccard", topK=4, shrink=0, normalize=True),
    dict(similarity="tanimoto", topK=10, shrink=5, normalize=False),
    dict(similarity="dice", topK=8, shrink=1, normalize=True),
    dict(similarity="tversky", topK=9, shrink=2, normalize=True, tversky_alpha=0.7, tversky_beta=1.5),
    dict(similarity="tversky", topK=30, shrink=0, normalize=False, tversky_alpha=1.0, tversky_beta=1.0),
    dict(similarity="cosine", topK=6, shrink=4, normalize=True, feature_weighting="BM25"),
    dict(similarity="cosine", topK=6, shrink=4, normalize=True, feature_weighting="TF-IDF"),
]


def tiny_matrix():
    rng = np.random.RandomState(20240)
    m = (rng.rand(40, 30) < 0.25) * rng.randint(1, 6, (40, 30))
    m[:, 11] = 0      # an item nobody rated
    m[7, :] = 0       # a user without ratings
    return sps.csr_matrix(m.astype(np.float32))


def make_tiny(out_path):
    from Base.IR_feature_weighting import TF_IDF, okapi_BM_25
    from Base.Similarity.Compute_Similarity_Python import Compute_Similarity_Python
    urm = tiny_matrix()
    arrays = {"urm": np.asarray(urm.todense(), dtype=np.float32), "cases": np.array(json.dumps(TINY_CASES))}
    for n, case in enumerate(TINY_CASES):
        args = dict(case)
        weighting = args.pop("feature_weighting", "none")
        data = urm
        if weighting == "BM25":
            data = sps.csr_matrix(okapi_BM_25(urm.astype(np.float32).T).T)
        elif weighting == "TF-IDF":
            data = sps.csr_matrix(TF_IDF(urm.astype(np.float32).T).T)
        W = Compute_Similarity_Python(data, **args).compute_similarity()
        arrays["W_%d" % n] = np.asarray(W.todense(), dtype=np.float64)
        if weighting != "none":
            arrays["weighted_%d" % n] = np.asarray(data.todense(), dtype=np.float64)
    np.savez_compressed(out_path, **arrays)
    print("wrote", out_path)


def logged_trials(reference, kind):
    """[(params, MAP@5)] of results.txt in file order"""
    text = open(os.path.join(reference, "experiments", "ItemKNNCFRecommender_%s_1M" % kind, "results.txt")).read()
    out = []
    for m in re.finditer(r"(\{[^\n]*\})\nCUTOFF: 5 - [^\n]*?MAP: ([0-9.]+),", text):
        out.append((json.loads(m.group(1)), float(m.group(2))))
    return out


def replay(train, valid, params):
    from Base.Evaluation.Evaluator import EvaluatorHoldout
    from Base.Similarity.Compute_Similarity_Python import Compute_Similarity_Python
    from KNN.ItemKNNCFRecommender import ItemKNNCFRecommender
    rec = ItemKNNCFRecommender(train.copy())
    args = dict(params)
    # the class's own fit() with the pure-Python similarity (its Cython extension is not built)
    rec.topK, rec.shrink = args["topK"], args["shrink"]
    rec.W_sparse = sps.csr_matrix(Compute_Similarity_Python(rec.URM_train, **args).compute_similarity())
    results, _ = EvaluatorHoldout(valid, cutoff_list=[5]).evaluateRecommender(rec)
    return float(results[5]["MAP"])


def make_trials(reference, out_path):
    train = sps.load_npz(os.path.join(GOLDEN, "Movielens1M_URM_train_small.npz")).tocsr()
    valid = sps.load_npz(os.path.join(GOLDEN, "Movielens1M_URM_validation.npz")).tocsr()
    trials = []
    for kind in KINDS:
        logged = logged_trials(reference, kind)
        best = json.load(open(os.path.join(reference, "experiments", "ItemKNNCFRecommender_%s_1M" % kind, "best_params.txt")))
        best_logged = [v for p, v in logged if p == best]
        rows = [("trial", p, v) for p, v in logged[:3]] + [("best", best, best_logged[0] if best_logged else None)]
        for role, params, value in rows:
            got = replay(train, valid, params)
            trials.append(dict(kind=kind, role=role, params=params, logged=value, replayed=got))
            print(kind, role, params, "logged", value, "replayed", got, flush=True)
    doc = dict(source="experiments/ItemKNNCFRecommender_<kind>_1M/results.txt and best_params.txt of the reference",
               metric="MAP", at=5, train="Movielens1M_URM_train_small.npz", validation="Movielens1M_URM_validation.npz",
               trials=trials)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--tiny-only", action="store_true")
    ap.add_argument("--trials-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    for name, kind in (("int", int), ("float", float), ("bool", bool), ("object", object)):
        if not hasattr(np, name):      # aliases the reference still uses, removed in numpy 1.24
            setattr(np, name, kind)
    if not a.trials_only:
        make_tiny(os.path.join(GOLDEN, "itemknn_tiny.npz"))
    if not a.tiny_only:
        make_trials(os.path.abspath(a.reference), os.path.join(GOLDEN, "itemknn_trial_logs_ml1m.json"))


if __name__ == "__main__":
    main()
