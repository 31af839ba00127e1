"""Writes tests/golden/evaluator_edge_expected.json: the reference's own Base/Evaluation/Evaluator.py (full 19-metric row)
on a tiny synthetic factor recommender built to hit the edge cases of the beyond-accuracy metrics:

  lists shorter than the cut-off (few unseen items left), a user with an empty list (user 0 scores -inf everywhere, as a
  cold user does under the MF contract; its RMSE, and so the mean, is NaN as in the reference), graded ratings, a
  recommended item without training interactions (pop = 0), users without test items (not evaluated, but counted by
  COVERAGE_USER), a test item that is also seen (-inf score: left out of RMSE).

The inputs (matrices, factors, cut-offs) go into the JSON next to the expected rows; the tests read only the JSON.

    python tools/make_eval_edge_golden.py REFERENCE_ROOT        # the reference checkout (its Base/ package)
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps
import numpy.ma  # noqa: F401  (must be imported before the alias shim below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "evaluator_edge_expected.json")
CUTOFFS = [1, 3, 5, 8]
COLD_USER = 0


def inputs():
    rng = np.random.RandomState(2024)
    n_users, n_items, k = 14, 12, 3
    train = (rng.rand(n_users, n_items) < 0.35).astype(np.float32)
    train[:, 11] = 0.0                          # item 11: no training interaction (pop = 0), high score below
    train[1, :10] = 1.0                         # users 1, 2: two unseen items, lists shorter than every cut-off > 2
    train[1, 10:] = 0.0
    train[2, :] = 1.0
    train[2, [3, 11]] = 0.0
    for u in range(n_users):                    # nobody else is cold
        if train[u].sum() == 0:
            train[u, u % 11] = 1.0
    test = ((rng.rand(n_users, n_items) < 0.3) * rng.randint(1, 6, size=(n_users, n_items))).astype(np.float32)
    test[0, :] = 0.0
    test[0, [2, 5]] = [4.0, 2.0]                # user 0 (all scores -inf) has test items but nothing to recommend
    test[[5, 9], :] = 0.0                       # users without test items
    test[3, 0] = 5.0
    train[3, 0] = 1.0                           # a test item that is also seen
    test[4, 11] = 3.0
    U = rng.randn(n_users, k).astype(np.float32)
    V = rng.randn(n_items, k).astype(np.float32)
    V[11] = np.abs(V[11]) * 3.0                 # the item without interactions ranks high for most users
    return train, test, U, V


def main(reference_root):
    train, test, U, V = inputs()
    np.int = int                                # numpy >= 1.24 dropped the aliases the reference uses
    np.bool = np.bool_
    np.float = float
    sys.path.insert(0, reference_root)
    from Base.BaseRecommender import BaseRecommender
    from Base.Evaluation.Evaluator import EvaluatorHoldout

    class Factors(BaseRecommender):
        RECOMMENDER_NAME = "edge"

        def _compute_item_score(self, user_id_array, items_to_compute=None):
            scores = U[user_id_array] @ V.T
            scores[np.asarray(user_id_array) == COLD_USER] = -np.inf
            return scores

    rec = Factors(sps.csr_matrix(train))
    got, _ = EvaluatorHoldout(sps.csr_matrix(test), CUTOFFS).evaluateRecommender(rec)
    lists = rec.recommend(np.arange(train.shape[0]), cutoff=max(CUTOFFS), remove_seen_flag=True)
    assert len(lists[0]) == 0 and len(lists[1]) == 2 and len(lists[2]) == 2
    assert any(11 in l for l in lists)
    expected = {str(c): {k: float(v) for k, v in d.items()} for c, d in got.items()}
    json.dump({"cutoffs": CUTOFFS, "cold_user": COLD_USER, "train": train.tolist(), "test": test.tolist(), "U": U.tolist(), "V": V.tolist(),
               "expected": expected}, open(OUT, "w"), indent=0)
    print("wrote", OUT, "COVERAGE_USER@5 =", expected["5"]["COVERAGE_USER"], "RMSE =", expected["5"]["RMSE"])


if __name__ == "__main__":
    main(sys.argv[1])
