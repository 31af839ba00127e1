"""Writes tests/golden/activity_study_expected.json: the per-user AP@cutoff of the reference's user-activity study
(MFLearned.py:122-133, fast_eval: the reference's own Base/BaseRecommender.recommend(all users, remove_seen_flag=True,
return_scores=True) and Base/Evaluation/metrics.py average_precision(is_relevant[:cutoff], relevant_items)) around a tiny
factor recommender, on a case built to hit:

  users in every activity bucket, the one the reference's figure drops included; a user whose count is exactly a bound; graded
  ratings in both train and test (the count is the sum of the stored values, not the nnz); a user with fewer unseen items than
  the cut-off (short list); a user without a hit; users without a test item (the reference's average_precision fails its own
  assert on 0/0 for them: stored as null, skipped by the study).

The same values with every user ranked only among its own candidates (test items + sampled negatives, the MF contract's
items_to_compute masking, one recommend call per user as Base/Evaluation/Evaluator.py:504-513 makes it) are stored for the
negative-sample evaluators.

The bucket rule lives in nested closures of MFLearned.py that cannot be imported; the study restates it
(ganmf_amd/studies.py) and tests/test_activity_study.py pins it with a hand-written table.  This tool only checks, with that
restatement, that the case populates every bucket.

The reference's ranking is not stable under ties (argpartition + argsort), so the case is only accepted when every user's
scores are, in float64, pairwise further apart than 1e-4 of the largest; the seed is redrawn otherwise.  The tests read only
the JSON.

    python tools/make_activity_study_golden.py REFERENCE_ROOT        # the reference checkout (its Base/ package)
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps
import numpy.ma  # noqa: F401  (must be imported before the alias shim below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "activity_study_expected.json")
CUTOFFS = [1, 5, 20]
BOUNDS = [8, 16, 30, 50]
N_USERS, N_ITEMS, K = 28, 30, 3
N_NEGATIVES = 9
NO_TEST, ON_BOUND, NO_HIT, SHORT = (0, 1), 2, 5, 6


def inputs(seed):
    rng = np.random.RandomState(seed)
    U = rng.randn(N_USERS, K).astype(np.float32)
    V = rng.randn(N_ITEMS, K).astype(np.float32)
    scores = U.astype(np.float64) @ V.astype(np.float64).T
    train = np.zeros((N_USERS, N_ITEMS), np.float32)
    test = np.zeros((N_USERS, N_ITEMS), np.float32)
    neg = np.zeros((N_USERS, N_ITEMS), np.float32)
    for u in range(N_USERS):
        n_train = 18 if u == SHORT else 2 if u in (NO_HIT, ON_BOUND) else rng.randint(1, 15)
        seen = rng.choice(N_ITEMS, size=n_train, replace=False)
        train[u, seen] = rng.randint(1, 6, size=n_train)                   # graded ratings
        unseen = np.setdiff1d(np.arange(N_ITEMS), seen)
        if u == NO_HIT:                                                    # the three lowest-scored unseen items: ranks 26..28
            picked = unseen[np.argsort(scores[u, unseen])][:3]
            rest = np.setdiff1d(unseen, picked)
        else:
            order = rng.permutation(unseen)
            picked, rest = order[:3], order[3:]
        test[u, picked] = rng.randint(1, 6, size=3)
        neg[u, rng.choice(rest, size=min(N_NEGATIVES, len(rest)), replace=False)] = 1.0
    for u in NO_TEST:
        test[u, :] = 0.0
    train[ON_BOUND, train[ON_BOUND] != 0] = 4.0                            # 4 + 4 in train, 3 + 3 + 2 in test: exactly BOUNDS[1]
    test[ON_BOUND, np.flatnonzero(test[ON_BOUND])] = [3.0, 3.0, 2.0]
    return train, test, neg, U, V


def well_separated(U, V):
    s = U.astype(np.float64) @ V.astype(np.float64).T
    for u in range(N_USERS):
        c = np.sort(s[u])
        if np.diff(c).min() <= 1e-4 * np.abs(c).max():
            return False
    return True


def covers(train, test):
    sys.path.insert(0, ROOT)
    from ganmf_amd.studies import activity_bucket
    counts = (train + test).sum(axis=1)
    bucket = activity_bucket(counts, BOUNDS)
    with_test = (test != 0).sum(axis=1) > 0
    return (counts[ON_BOUND] == BOUNDS[1] and bucket[ON_BOUND] == 2 and bucket[SHORT] == len(BOUNDS)
            and set(bucket[with_test]) == set(range(len(BOUNDS) + 1)) and np.any(counts != (train != 0).sum(axis=1) + (test != 0).sum(axis=1)))


def main(reference_root):
    seed = 2026
    while True:
        train, test, neg, U, V = inputs(seed)
        if well_separated(U, V) and covers(train, test):
            break
        seed += 1
    np.int = int                                # numpy >= 1.24 dropped the aliases the reference uses
    np.bool = np.bool_
    np.float = float
    sys.path.insert(0, reference_root)
    from Base.BaseRecommender import BaseRecommender
    from Base.Evaluation.metrics import average_precision

    class Factors(BaseRecommender):
        RECOMMENDER_NAME = "activity_study"

        def _compute_item_score(self, user_id_array, items_to_compute=None):
            if items_to_compute is None:
                return U[user_id_array] @ V.T
            masked = np.full((len(user_id_array), V.shape[0]), -np.inf, dtype=np.float32)
            masked[:, items_to_compute] = U[user_id_array] @ V[items_to_compute].T
            return masked

    rec = Factors(sps.csr_matrix(train))
    URM_test = sps.csr_matrix(test)
    rank = sps.csr_matrix(((test != 0) | (neg != 0)).astype(np.float32))
    rank.sort_indices()
    users = np.arange(N_USERS)
    top = max(CUTOFFS)
    lists, _ = rec.recommend(users, remove_seen_flag=True, cutoff=top, return_scores=True)
    cand_lists = [rec.recommend(np.atleast_1d(u), cutoff=top, remove_seen_flag=True,
                                items_to_compute=rank.indices[rank.indptr[u]:rank.indptr[u + 1]])[0] for u in users]
    assert len(lists[SHORT]) == N_ITEMS - 18 < top and all(len(lists[u]) == top for u in users if u != SHORT and (train[u] != 0).sum() <= 10)

    def ap(ranked, cutoff):
        out = []
        for u in users:
            relevant_items = URM_test.indices[URM_test.indptr[u]:URM_test.indptr[u + 1]]
            if len(relevant_items) == 0:
                out.append(None)
                continue
            is_relevant = np.isin(ranked[u], relevant_items, assume_unique=True)
            out.append(float(average_precision(is_relevant[:cutoff], relevant_items)))
        return out

    full = {str(c): ap(lists, c) for c in CUTOFFS}
    cand = {str(c): ap(cand_lists, c) for c in CUTOFFS}
    assert full[str(top)][NO_HIT] == 0.0 and all(full[str(top)][u] is None for u in NO_TEST)
    assert sum(v is None for v in full[str(top)]) == len(NO_TEST) and sum(v is not None and v > 0 for v in full[str(top)]) >= 20
    json.dump({"seed": seed, "cutoffs": CUTOFFS, "bounds": BOUNDS, "train": train.tolist(), "test": test.tolist(),
               "negative": neg.tolist(), "U": U.tolist(), "V": V.tolist(),
               "users": {"no_test": list(NO_TEST), "on_bound": ON_BOUND, "no_hit": NO_HIT, "short_list": SHORT},
               "ap": full, "ap_candidates": cand}, open(OUT, "w"), indent=0)
    print("wrote", OUT, "seed", seed, "mean AP@%d =" % top, np.mean([v for v in full[str(top)] if v is not None]))


if __name__ == "__main__":
    main(sys.argv[1])
