"""Writes tests/golden/evaluator_ignore_inputs.npz and evaluator_ignore_expected.json: what the reference's own EvaluatorHoldout
and EvaluatorNegativeItemSample (Base/Evaluation/Evaluator.py, full 19/20-metric row) return with `diversity_object`,
`ignore_items` and `ignore_users` around a small factor recommender whose _compute_item_score is U[ids] @ V.T in float32 (the
way evaluator_expected.json was made); for the negative-sample protocol the recommender applies the MF contract's
`items_to_compute` masking (Base/BaseMatrixFactorizationRecommender.py:113-119).

Inputs: 240 users x 181 items, k = 16, train density about 8 %, graded test ratings 1..5, 30 negatives per user;
  ignore_items   23 ids: three of the ten most popular items, items that are some user's test items, one id twice (the reference's
                 Coverage_Item subtracts len(ignore_items));
  ignore_users   17 ids, two of them below minRatingsPerUser = 2;
  D              [181, 181], NOT symmetric, entries q / 256 with integer q in [0, 256], stored as the uint16 numerators: every row
                 sum the reference forms is exact in float32 and float64 alike, so recorded and recomputed DIVERSITY_SIMILARITY can
                 differ only by the final divisions and the order of the mean over the users;
  cut-offs       [2, 5, 20]: at 2 the metric is D[l_0, l_1] / 2, which pins the skipped last row and the asymmetry.

The reference's ranking is not stable under ties and a GPU scores in another summation order, so a case is accepted only when
every evaluated user has at least 21 unmasked items under every mask recorded here (unseen; unseen and not ignored; its unseen
candidates) and the smallest gap between neighbours among its 21 best unmasked float64 scores is at least 1e-4 x max|score|.  A user
whose random factor row misses that is given the next row of the same stream; a case that still misses is redrawn with the next
seed.

Recorded rows: hold-out with all three arguments, with each alone, and negative-sample with ignore_users + diversity_object
(ignore_items = None there: the reference resets the recommender's ignore list inside its user loop, Evaluator.py:530, so only its
first user would be filtered -- a quirk ganmf_amd.evaluation does not copy).

    python tools/make_golden_ignore.py REFERENCE_ROOT        # the reference checkout (its Base/ package)
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps
import numpy.ma  # noqa: F401  (must be imported before the alias shim below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CUTOFFS = [2, 5, 20]
MIN_RATINGS = 2
N_USERS, N_ITEMS, K = 240, 181, 16
N_NEGATIVES = 30
NEED = max(CUTOFFS) + 1


def separated(row_scores, allowed):
    s = np.sort(row_scores[allowed])[::-1][:NEED]
    return len(s) >= NEED and -np.diff(s).min() >= 1e-4 * np.abs(row_scores).max()


def inputs(seed):
    rng = np.random.RandomState(seed)
    popularity = rng.rand(N_ITEMS) ** 2
    train = (rng.rand(N_USERS, N_ITEMS) < 0.16 * popularity / popularity.mean() * 0.5).astype(np.float32)
    test = np.zeros((N_USERS, N_ITEMS), np.float32)
    neg = np.zeros((N_USERS, N_ITEMS), np.float32)
    for u in range(N_USERS):
        unseen = np.flatnonzero(train[u] == 0)
        n_test = rng.randint(2, 7)
        picked = rng.choice(unseen, size=n_test + N_NEGATIVES, replace=False)
        test[u, picked[:n_test]] = rng.randint(1, 6, size=n_test)
        neg[u, picked[n_test:]] = 1.0
    below = [11, 97]                                                   # below minRatingsPerUser: one test item, none
    test[below[0], np.flatnonzero(test[below[0]])[1:]] = 0.0
    test[below[1], :] = 0.0
    pop_order = np.argsort(-train.sum(axis=0), kind="stable")
    tested = np.flatnonzero((test != 0).sum(axis=0) > 0)
    ignore = list(pop_order[[0, 3, 7]])
    ignore += [i for i in tested if i not in ignore][:8]
    ignore += [i for i in rng.permutation(N_ITEMS) if i not in ignore][:22 - len(ignore)]
    ignore_items = np.array(ignore + [ignore[4]], dtype=np.int64)      # 22 distinct ids, one of them twice
    others = [u for u in rng.permutation(N_USERS) if u not in below][:15]
    ignore_users = np.array(sorted(others[:7]) + below + others[7:], dtype=np.int64)
    D = rng.randint(0, 257, size=(N_ITEMS, N_ITEMS)).astype(np.uint16)
    V = rng.randn(N_ITEMS, K).astype(np.float32)
    U = np.zeros((N_USERS, K), np.float32)
    ignored = np.zeros(N_ITEMS, bool)
    ignored[ignore_items] = True
    for u in range(N_USERS):
        unseen = train[u] == 0
        for _ in range(200):
            U[u] = rng.randn(K).astype(np.float32)
            s = U[u].astype(np.float64) @ V.astype(np.float64).T
            if (separated(s, unseen) and separated(s, unseen & ~ignored)
                    and separated(s, unseen & ((test[u] != 0) | (neg[u] != 0)))):
                break
        else:
            return None
    return dict(train=train, test=test, negative=neg, U=U, V=V, D=D, ignore_items=ignore_items, ignore_users=ignore_users)


def main(reference_root):
    seed = 2027
    while True:
        g = inputs(seed)
        if g is not None:
            break
        seed += 1
    train, test, neg, U, V = g["train"], g["test"], g["negative"], g["U"], g["V"]
    ignore_items, ignore_users = g["ignore_items"], g["ignore_users"]
    assert len(ignore_items) == 23 and len(set(ignore_items.tolist())) == 22 and len(ignore_users) == 17
    top10 = set(np.argsort(-train.sum(axis=0), kind="stable")[:10].tolist())
    assert len(top10 & set(ignore_items.tolist())) >= 3
    assert ((test != 0).sum(axis=0)[np.unique(ignore_items)] > 0).sum() >= 5
    assert ((test != 0).sum(axis=1)[ignore_users] < MIN_RATINGS).sum() == 2
    assert not np.array_equal(g["D"], g["D"].T)
    # the reference gets the float64 matrix, so that its divisions and its running sum are float64 ones (on a float32 matrix
    # they are float32 or float64 depending on the numpy version's scalar promotion); the values are those of the float32 matrix
    # the library uses, exactly
    D64 = g["D"].astype(np.float64) / 256.0
    assert np.array_equal(D64.astype(np.float32).astype(np.float64), D64)

    np.int = int                                # numpy >= 1.24 dropped the aliases the reference uses
    np.bool = np.bool_
    np.float = float
    sys.path.insert(0, reference_root)
    from Base.BaseRecommender import BaseRecommender
    from Base.Evaluation.Evaluator import EvaluatorHoldout, EvaluatorNegativeItemSample
    from Base.Evaluation.metrics import Diversity_similarity

    class Factors(BaseRecommender):
        RECOMMENDER_NAME = "ignore_fixture"

        def _compute_item_score(self, user_id_array, items_to_compute=None):
            if items_to_compute is None:
                return U[user_id_array] @ V.T
            masked = np.full((len(user_id_array), V.shape[0]), -np.inf, dtype=np.float32)
            masked[:, items_to_compute] = U[user_id_array] @ V[items_to_compute].T
            return masked

    rec = Factors(sps.csr_matrix(train))
    URM_test, URM_neg = sps.csr_matrix(test), sps.csr_matrix(neg)

    def row(evaluator):
        got, _ = evaluator.evaluateRecommender(rec)
        assert not rec.items_to_ignore_flag
        return {str(c): {k: float(v) for k, v in d.items()} for c, d in got.items()}

    def holdout(**kw):
        if "diversity_object" in kw:
            kw["diversity_object"] = Diversity_similarity(D64)
        return row(EvaluatorHoldout(URM_test, CUTOFFS, minRatingsPerUser=MIN_RATINGS, **kw))

    expected = {
        "holdout_all": holdout(diversity_object=True, ignore_items=ignore_items, ignore_users=ignore_users),
        "holdout_diversity": holdout(diversity_object=True),
        "holdout_ignore_items": holdout(ignore_items=ignore_items),
        "holdout_ignore_users": holdout(ignore_users=ignore_users),
        "negative_users_diversity": row(EvaluatorNegativeItemSample(URM_test, URM_neg, CUTOFFS, minRatingsPerUser=MIN_RATINGS,
                                                                    diversity_object=Diversity_similarity(D64),
                                                                    ignore_users=ignore_users)),
    }
    assert len(expected["holdout_all"]["5"]) == 20 and len(expected["holdout_ignore_items"]["5"]) == 19
    np.savez_compressed(os.path.join(GOLDEN, "evaluator_ignore_inputs.npz"), train=train.astype(np.uint8), test=test.astype(np.uint8),
                        negative=neg.astype(np.uint8), U=U, V=V, D=g["D"], ignore_items=ignore_items, ignore_users=ignore_users)
    json.dump({"seed": seed, "cutoffs": CUTOFFS, "min_ratings_per_user": MIN_RATINGS, "expected": expected},
              open(os.path.join(GOLDEN, "evaluator_ignore_expected.json"), "w"), indent=0)
    print("wrote the ignore fixture, seed", seed, "DIVERSITY_SIMILARITY@2 =", expected["holdout_all"]["2"]["DIVERSITY_SIMILARITY"],
          "COVERAGE_ITEM@20 =", expected["holdout_all"]["20"]["COVERAGE_ITEM"])


if __name__ == "__main__":
    main(sys.argv[1])
