"""Writes tests/golden/negative_sample_expected.json: the reference's own EvaluatorNegativeItemSample
(Base/Evaluation/Evaluator.py:419-590, full 19-metric row) around a tiny factor recommender that applies the MF contract's
`items_to_compute` masking (Base/BaseMatrixFactorizationRecommender.py:113-119), on a case built to hit:

  an item stored in both the test and the negative matrix (URM_items_to_rank keeps it once), a user without negatives, a user
  whose candidates are all seen (empty list; its RMSE, and so the mean, is NaN as in the reference), a user with two candidates
  (fewer than every cut-off above 2), users below minRatingsPerUser (one test item, none), graded ratings, a test item that is
  also seen (-inf score: left out of RMSE).

The reference's ranking is not stable under ties (argpartition + argsort), so the case is only accepted when every user's
candidate scores are, in float64, pairwise further apart than 1e-4 of the largest; the seed is redrawn otherwise.

The inputs (matrices, factors, cut-offs, the reference's URM_items_to_rank) go into the JSON next to the expected rows; the
tests read only the JSON.

    python tools/make_negative_sample_golden.py REFERENCE_ROOT        # the reference checkout (its Base/ package)
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps
import numpy.ma  # noqa: F401  (must be imported before the alias shim below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "negative_sample_expected.json")
CUTOFFS = [1, 3, 5, 8]
MIN_RATINGS = 2
N_USERS, N_ITEMS, K = 18, 40, 3
N_NEGATIVES = 9


def inputs(seed):
    rng = np.random.RandomState(seed)
    train = (rng.rand(N_USERS, N_ITEMS) < 0.2).astype(np.float32)
    test = np.zeros((N_USERS, N_ITEMS), np.float32)
    neg = np.zeros((N_USERS, N_ITEMS), np.float32)
    for u in range(N_USERS):
        unseen = np.flatnonzero(train[u] == 0)
        picked = rng.choice(unseen, size=3 + N_NEGATIVES, replace=False)
        test[u, picked[:3]] = rng.randint(1, 6, size=3)               # graded ratings
        neg[u, picked[3:]] = 1.0
        if train[u].sum() == 0:                                        # nobody is cold
            train[u, np.setdiff1d(np.arange(N_ITEMS), picked)[0]] = 1.0
    test[0, :] = 0.0                                                   # users 0, 1: below minRatingsPerUser (no / one test item)
    one = np.flatnonzero(test[1])
    test[1, one[1:]] = 0.0
    seen3 = np.flatnonzero(train[3])[0]                                # user 3: a test item that is also seen
    test[3, seen3] = 4.0
    both4 = np.flatnonzero(test[4])[0]                                 # user 4: an item stored in both matrices
    neg[4, both4] = 1.0
    neg[5, :] = 0.0                                                    # user 5: no negatives
    train[6, (test[6] != 0) | (neg[6] != 0)] = 1.0                     # user 6: every candidate is seen
    keep = np.flatnonzero(test[7])[:2]                                 # user 7: two candidates, both test items
    test[7, np.setdiff1d(np.flatnonzero(test[7]), keep)] = 0.0
    neg[7, :] = 0.0
    U = rng.randn(N_USERS, K).astype(np.float32)
    V = rng.randn(N_ITEMS, K).astype(np.float32)
    return train, test, neg, U, V


def well_separated(test, neg, U, V):
    s = U.astype(np.float64) @ V.astype(np.float64).T
    for u in range(N_USERS):
        c = np.sort(s[u, (test[u] != 0) | (neg[u] != 0)])
        if len(c) > 1 and np.diff(c).min() <= 1e-4 * np.abs(c).max():
            return False
    return True


def main(reference_root):
    seed = 2025
    while True:
        train, test, neg, U, V = inputs(seed)
        if well_separated(test, neg, U, V):
            break
        seed += 1
    np.int = int                                # numpy >= 1.24 dropped the aliases the reference uses
    np.bool = np.bool_
    np.float = float
    sys.path.insert(0, reference_root)
    from Base.BaseRecommender import BaseRecommender
    from Base.Evaluation.Evaluator import EvaluatorNegativeItemSample

    class Factors(BaseRecommender):
        RECOMMENDER_NAME = "negative_sample"

        def _compute_item_score(self, user_id_array, items_to_compute=None):
            if items_to_compute is None:
                return U[user_id_array] @ V.T
            masked = np.full((len(user_id_array), V.shape[0]), -np.inf, dtype=np.float32)
            masked[:, items_to_compute] = U[user_id_array] @ V[items_to_compute].T
            return masked

    rec = Factors(sps.csr_matrix(train))
    ev = EvaluatorNegativeItemSample(sps.csr_matrix(test), sps.csr_matrix(neg), CUTOFFS, minRatingsPerUser=MIN_RATINGS)
    got, _ = ev.evaluateRecommender(rec)
    rank = ev.URM_items_to_rank.tocsr()
    rank.sort_indices()
    per_user = np.ediff1d(rank.indptr)
    assert per_user[4] == 3 + N_NEGATIVES and per_user[5] == 3 and per_user[7] == 2 and per_user[3] == 4 + N_NEGATIVES
    assert sorted(ev.usersToEvaluate) == list(range(2, N_USERS))
    lists = [rec.recommend(np.atleast_1d(u), cutoff=max(CUTOFFS), remove_seen_flag=True,
                           items_to_compute=rank.indices[rank.indptr[u]:rank.indptr[u + 1]])[0] for u in range(N_USERS)]
    assert len(lists[6]) == 0 and len(lists[7]) == 2 and len(lists[5]) == 3
    expected = {str(c): {k: float(v) for k, v in d.items()} for c, d in got.items()}
    assert len(expected[str(CUTOFFS[0])]) == 19
    json.dump({"seed": seed, "cutoffs": CUTOFFS, "min_ratings_per_user": MIN_RATINGS, "train": train.tolist(), "test": test.tolist(),
               "negative": neg.tolist(), "U": U.tolist(), "V": V.tolist(),
               "items_to_rank": {"indptr": rank.indptr.tolist(), "indices": rank.indices.tolist()},
               "both_user": 4, "expected": expected}, open(OUT, "w"), indent=0)
    print("wrote", OUT, "seed", seed, "MAP@5 =", expected["5"]["MAP"], "RMSE =", expected["5"]["RMSE"])


if __name__ == "__main__":
    main(sys.argv[1])
