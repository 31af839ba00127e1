"""Hold-out and negative-sample evaluation -- the consumers of the scores (protocols of Base/Evaluation/Evaluator.py:214-414,
EvaluatorHoldout*, and :419-590, EvaluatorNegativeItemSample*: each user ranked among its own candidates; with the
metrics of Base/Evaluation/metrics.py).  The GANMF callers read `results_dic[cutoff][metric]` (early stopping:
cut-off 5, Utils_.py:64).

By default both evaluators return the eleven accuracy values of METRICS.  With `full_metrics=True` they return the
reference's whole row, FULL_METRICS in the reference's key order (Evaluator.py:20-40).  The reference's three further
constructor arguments (Evaluator.py:119-122) are keywords after `full_metrics`:
  diversity_object  an object with an `item_diversity_matrix` attribute (metrics.py:405-452 Diversity_similarity) or a plain
                    [n_items, n_items] array D with values in [0, 1] (asserted, as there).  The key DIVERSITY_SIMILARITY is in the
                    rows iff one was given: after AVERAGE_POPULARITY in a full row (the reference's place), else appended to the
                    eleven.  D is rounded to float32 ONCE and every route -- per user, blocks, device -- uses the rounded matrix.
                    Per list l of length L at a cut-off: sum over i = 0 .. L-2 (the last item's row is never visited; D need not
                    be symmetric) and j != i of D[l_i, l_j], divided by L (L - 1); the mean over the evaluated users.  A list with
                    L < 2 has value 0 and still counts in the mean (the reference raises ZeroDivisionError there).
  ignore_items      set_items_to_ignore(ignore_items) on the recommender around the whole evaluation (reset in a finally), every
                    `recommend` / device call with remove_CustomItems_flag (Evaluator.py:369-370, 410-411, 275): the items are never
                    recommended and, scoring -inf, do not count in RMSE; the relevant items are not filtered.  COVERAGE_ITEM divides
                    by n_items - len(ignore_items) (`len`: a repeated id counts twice, metrics.py:36-46); Gini, Herfindahl and
                    Shannon clear the ignored bins (:151-165, 201-215, 251-269).
  ignore_users      usersToEvaluate minus the list, ascending (Evaluator.py:171-176); COVERAGE_USER divides by
                    n_users - len(ignore_users) (metrics.py:64-73).
Deviation: the reference's EvaluatorNegativeItemSample resets the recommender's ignore list INSIDE its user loop
(Evaluator.py:530), so only the first evaluated user is filtered there; the negative-sample evaluators here apply ignore_items
to every user.

Metric definitions (one user, a ranked list `L` cut at c, test items `T` with ratings `w`, hit flags `h_i = [L_i in T]`):
  PRECISION = sum(h)/|L|      PRECISION_RECALL_MIN_DEN = sum(h)/min(|T|,|L|)      RECALL = sum(h)/|T|
  HIT_RATE = sum(h)           MRR = 1/rank of the first hit        ARHR = sum_i h_i/i
  MAP = sum_i h_i * (hits up to i)/i / min(|T|,|L|)
  ROC_AUC = share of (hit, miss) pairs of the list ranked in the right order (1 when the list has no miss)
  NDCG = DCG(L)/DCG(best |L| of T),  DCG = sum_i (2^{w_i}-1)/ln(i+1)
  RMSE over the test items whose score is finite (seen items carry -inf and do not count)
Every user contributes the same weight; values are means over the evaluated users; F1 is formed from the means.
Beyond accuracy (full_metrics; `pop` = per-item nnz of recommender.get_URM_train() at evaluation time, count_c[i] = number of
evaluated users with i in L; `beyond_accuracy_metrics` finishes them for every route, metrics.py:30-551):
  NOVELTY = mean over users of sum_{i in L, pop_i > 0} -log2(pop_i/sum(pop))/len(pop)
  AVERAGE_POPULARITY = mean over users of mean_{i in L} pop_i/max(pop)  (an empty list adds 0)
  COVERAGE_ITEM = share of items with count_c > 0;  COVERAGE_USER = users with a non-empty L / rows of URM_test
  DIVERSITY_GINI, SHANNON_ENTROPY (over the non-zero counts), DIVERSITY_HERFINDAHL, DIVERSITY_MEAN_INTER_LIST from count_c

`RankedListMetrics` computes the accuracy values for one list in one pass over the hit positions.  Where the reference's
evaluator works in float32 (hit counts divided in float32, the DCG sums, and therefore its running sums) this one
does too, so that the two agree to the last digits on the reference's golden outputs (tests/test_evaluator.py)."""
import itertools

import numpy as np
import scipy.sparse as sps

METRICS = ("ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "F1",
           "HIT_RATE", "ARHR", "RMSE")
BEYOND_ACCURACY = ("NOVELTY", "AVERAGE_POPULARITY", "DIVERSITY_MEAN_INTER_LIST", "DIVERSITY_HERFINDAHL", "COVERAGE_ITEM",
                   "COVERAGE_USER", "DIVERSITY_GINI", "SHANNON_ENTROPY")
FULL_METRICS = METRICS + BEYOND_ACCURACY
_SUMMED = tuple(m for m in METRICS if m != "F1")
DIVERSITY = "DIVERSITY_SIMILARITY"       # present in a row iff the evaluator was given a diversity_object


def get_result_string(results_run, n_decimals=7):
    """'CUTOFF: c - NAME: value, NAME: value, \n' per cut-off, the line format the reference's drivers log."""
    lines = []
    for cutoff, per_metric in results_run.items():
        fields = "".join("%s: %.*f, " % (name, n_decimals, value) for name, value in per_metric.items())
        lines.append("CUTOFF: %s - %s\n" % (cutoff, fields))
    return "".join(lines)


def item_popularity(URM_train):
    """Per-column nnz of URM_train with explicit zeros dropped (metrics.py Novelty / AveragePopularity __init__: CSC,
    eliminate_zeros, ediff1d of indptr), counted straight from the stored entries without building the CSC copy."""
    URM_train = sps.csr_matrix(URM_train)
    return np.bincount(URM_train.indices[URM_train.data != 0], minlength=URM_train.shape[1])


def _train_matrix(recommender_object):
    """URM_train of the recommender at evaluation time (Evaluator.py:250); read in place where the recommender keeps it,
    since get_URM_train() is a copy of that attribute"""
    held = getattr(recommender_object, "URM_train", None)
    return held if sps.issparse(held) else recommender_object.get_URM_train()


def popularity_weights(pop):
    """(novelty term, normalised popularity) per item in float64, as metrics.py forms them: -log2(pop/sum(pop))/len(pop)
    (0 where pop = 0: Novelty drops zero probabilities) and pop/max(pop).  The evaluators only gather and add these."""
    pop = np.asarray(pop)
    probability = pop / pop.sum()
    novelty = np.zeros(len(pop), dtype=np.float64)
    nz = probability != 0
    novelty[nz] = -np.log2(probability[nz]) / len(pop)
    return novelty, pop / pop.max()


def beyond_accuracy_metrics(counts, novelty_sum, popularity_sum, n_nonempty, n_eval, cutoff, n_items, n_users, ignore_items=None,
                            ignore_users=None):
    """The eight beyond-accuracy values of one cut-off in float64, from the per-item recommendation counts `counts`
    ([n_items], summed over all evaluated users) and the sums over the users of the novelty terms, of the mean normalised
    popularity of each list and of the non-empty lists.  Verbatim metrics.py get_metric_value.  `ignore_items` / `ignore_users`
    (the evaluator's lists): the coverage denominators shrink by their LENGTHS, and Herfindahl, Gini and Shannon clear the
    ignored items' bins first; Novelty, AveragePopularity and MeanInterList do not know about the lists."""
    counts = np.asarray(counts, dtype=np.float64)
    n_ignored_items = 0 if ignore_items is None else len(ignore_items)
    n_ignored_users = 0 if ignore_users is None else len(ignore_users)
    seen_counts = counts
    if n_ignored_items:
        counts = counts.copy()
        counts[np.asarray(ignore_items, dtype=np.int64)] = 0.0
    out = {}
    out["NOVELTY"] = novelty_sum / n_eval if n_eval else 0.0
    out["AVERAGE_POPULARITY"] = popularity_sum / n_eval if n_eval else 0.0
    # Diversity_MeanInterList (:536-551): the cut-off itself, not the list length
    if n_eval == 0:
        out["DIVERSITY_MEAN_INTER_LIST"] = 1.0
    else:
        cooccurrences_cumulative = np.sum(seen_counts ** 2) - n_eval * cutoff
        all_user_couples_count = n_eval ** 2 - n_eval
        diversity_cumulative = all_user_couples_count - cooccurrences_cumulative / cutoff
        with np.errstate(divide="ignore", invalid="ignore"):
            out["DIVERSITY_MEAN_INTER_LIST"] = diversity_cumulative / all_user_couples_count
    # Diversity_Herfindahl (:210-224)
    if counts.sum() != 0:
        out["DIVERSITY_HERFINDAHL"] = 1 - np.sum((counts / counts.sum()) ** 2)
    else:
        out["DIVERSITY_HERFINDAHL"] = np.nan
    out["COVERAGE_ITEM"] = (seen_counts > 0).sum() / (n_items - n_ignored_items)   # Coverage_Item (:45-46)
    out["COVERAGE_USER"] = n_nonempty / (n_users - n_ignored_users)                # Coverage_User (:72-73)
    nonzero = counts[counts != 0]
    # Gini_Diversity (:160-178)
    n = len(nonzero)
    srt = np.sort(nonzero)
    index = np.arange(1, n + 1)
    out["DIVERSITY_GINI"] = 2 * np.sum((n + 1 - index) / (n + 1) * srt / np.sum(srt))
    # Shannon_Entropy (:260-280)
    probability = nonzero / nonzero.sum()
    out["SHANNON_ENTROPY"] = -np.sum(probability * np.log2(probability))
    return {k: float(v) for k, v in out.items()}


class _FullSums(object):
    """Per cut-off: the [n_items] recommendation counts and the three per-user sums of the beyond-accuracy metrics."""

    def __init__(self, cutoffs, n_items):
        self.counts = {c: np.zeros(n_items, dtype=np.int64) for c in cutoffs}
        self.novelty = dict.fromkeys(cutoffs, 0.0)
        self.popularity = dict.fromkeys(cutoffs, 0.0)
        self.nonempty = dict.fromkeys(cutoffs, 0)

    def rows(self, results, n_eval, cutoffs, n_items, n_users, ignore_items=None, ignore_users=None):
        """results[c] in the reference's key order: the accuracy values as given, then the beyond-accuracy ones, DIVERSITY_SIMILARITY
        (when results[c] has it) after AVERAGE_POPULARITY"""
        for c in cutoffs:
            row = {m: results[c][m] for m in METRICS}
            for name, value in beyond_accuracy_metrics(self.counts[c], self.novelty[c], self.popularity[c], self.nonempty[c], n_eval, c,
                                                       n_items, n_users, ignore_items, ignore_users).items():
                row[name] = value
                if name == "AVERAGE_POPULARITY" and DIVERSITY in results[c]:
                    row[DIVERSITY] = results[c][DIVERSITY]
            results[c] = row
        return results


def list_diversity(D, items, cutoffs):
    """Intra-list diversity (metrics.py:405-452) of the ranked lists `items` ([n, K] ids, -1 padded at the end) at every cut-off:
    [n, len(cutoffs)] float64.  With L = min(c, valid ids of the row): the sum of D[l_i, l_j] over i = 0 .. L-2 and j != i, j < L,
    divided by L (L - 1); 0 when L < 2."""
    items = np.asarray(items)
    n, K = items.shape
    length = (items >= 0).sum(axis=1)
    out = np.zeros((n, len(cutoffs)), dtype=np.float64)
    for ci, c in enumerate(cutoffs):
        c = min(int(c), K)
        if c < 2 or n == 0:
            continue
        pos = np.arange(c)
        off_diagonal = pos[:, None] != pos[None, :]
        step = max(1, int(4e6) // (c * c))
        for lo in range(0, n, step):
            ids = items[lo:lo + step, :c]
            ids = np.where(ids >= 0, ids, 0)
            L = np.minimum(length[lo:lo + step], c)
            keep = ((pos[None, :, None] + 2 <= L[:, None, None]) & (pos[None, None, :] + 1 <= L[:, None, None]) & off_diagonal[None])
            total = (D[ids[:, :, None], ids[:, None, :]].astype(np.float64) * keep).sum(axis=(1, 2))
            out[lo:lo + step, ci] = np.where(L >= 2, total / np.maximum(L * (L - 1), 1), 0.0)
    return out


class DiversitySimilarity(object):
    """The reference's Diversity_similarity metric object (metrics.py:405-452) with the L < 2 rule of this package: a list of fewer
    than two items adds 0 (the reference divides by zero) and counts as an evaluated user."""

    def __init__(self, item_diversity_matrix):
        D = np.asarray(item_diversity_matrix)
        assert np.all(D >= 0.0) and np.all(D <= 1.0), "item_diversity_matrix contains value greater than 1.0 or lower than 0.0"
        self.item_diversity_matrix = D
        self.n_evaluated_users = 0
        self.diversity = 0.0

    def add_recommendations(self, recommended_items_ids):
        ids = np.asarray(recommended_items_ids, dtype=np.int64).reshape(1, -1)
        if ids.shape[1] >= 2:
            self.diversity += float(list_diversity(self.item_diversity_matrix, ids, [ids.shape[1]])[0, 0])
        self.n_evaluated_users += 1

    def get_metric_value(self):
        return self.diversity / self.n_evaluated_users if self.n_evaluated_users else 0.0


class RankedListMetrics(object):
    """Accuracy metrics of one user's ranked list against that user's test items.

    `test_items` / `test_ratings`: the stored entries of the user's URM_test row.  `__call__(recommended, c)` returns a
    dict over the metric names for the list cut at c.  `dtype=np.float64`: the same values in float64 throughout, as
    EvaluatorHoldoutFast and the device form them (only the ratings' powers of two and the logarithms stay float32, as everywhere)
    -- the per-user values of `evaluateRecommenderByGroup`."""

    def __init__(self, test_items, test_ratings, max_cutoff, dtype=np.float32):
        self._exact = np.dtype(dtype) == np.float64
        order = np.argsort(test_items, kind="stable")
        self._items = np.asarray(test_items)[order]
        self._ratings = np.asarray(test_ratings)[order]
        self.n_test = int(self._items.shape[0])
        # DCG discounts ln(rank + 1), rank = 1..max_cutoff, and the user's best possible gains, both float32
        self._ln_rank = np.log(np.arange(max_cutoff, dtype=np.float32) + 2)
        best_first = np.sort(np.asarray(test_ratings))[::-1][:max_cutoff]
        self._ideal_terms = (np.power(2, best_first.astype(np.float32)) - 1) / self._ln_rank[:best_first.shape[0]]
        if self._exact:
            self._disc = 1.0 / self._ln_rank.astype(np.float64)
            self._ideal_cum = np.cumsum((np.power(2.0, best_first.astype(np.float32)).astype(np.float64) - 1.0)
                                        * self._disc[:best_first.shape[0]])

    def match(self, recommended):
        """(hit flags, rating of each hit else 0) for the ranked ids."""
        recommended = np.asarray(recommended, dtype=self._items.dtype if self.n_test else np.int64)
        if self.n_test == 0 or recommended.shape[0] == 0:
            return np.zeros(recommended.shape[0], dtype=bool), np.zeros(recommended.shape[0], dtype=np.float32)
        slot = np.minimum(np.searchsorted(self._items, recommended), self.n_test - 1)
        hit = self._items[slot] == recommended
        return hit, np.where(hit, self._ratings[slot], 0).astype(np.float32)

    def _call_float64(self, hit, gain, c):
        hit, gain = hit[:c], gain[:c]
        n = int(hit.shape[0])
        at = np.flatnonzero(hit)
        n_hit = int(at.shape[0])
        n_miss = n - n_hit
        out = dict.fromkeys(_SUMMED, 0.0)
        out["HIT_RATE"] = float(n_hit)
        out["RECALL"] = n_hit / self.n_test if self.n_test else float("nan")
        if n:
            out["PRECISION"] = n_hit / n
            out["PRECISION_RECALL_MIN_DEN"] = n_hit / max(min(self.n_test, n), 1)
        if n_miss == 0:
            out["ROC_AUC"] = 1.0
        elif n_hit:
            out["ROC_AUC"] = int(((n - 1 - at) - (n_hit - 1 - np.arange(n_hit))).sum()) / (n_hit * n_miss)
        if n_hit:
            rank = at + 1.0
            out["MRR"] = float(1.0 / rank[0])
            out["ARHR"] = float((1.0 / rank).sum())
            out["MAP"] = float((np.arange(1, n_hit + 1, dtype=np.float64) / rank).sum()) / min(self.n_test, n)
            dcg = float(((np.power(2.0, gain[at].astype(np.float32)).astype(np.float64) - 1.0) * self._disc[at]).sum())
            if dcg > 0.0:
                out["NDCG"] = dcg / float(self._ideal_cum[min(n, self._ideal_cum.shape[0]) - 1])
        return out

    def __call__(self, hit, gain, c):
        if self._exact:
            return self._call_float64(hit, gain, c)
        hit, gain = hit[:c], gain[:c]
        n = int(hit.shape[0])
        at = np.flatnonzero(hit)                       # 0-based ranks of the hits
        n_hit = int(at.shape[0])
        hits32 = np.float32(n_hit)
        out = dict.fromkeys(_SUMMED, 0.0)
        out["HIT_RATE"] = n_hit
        out["RECALL"] = hits32 / self.n_test
        if n:
            out["PRECISION"] = hits32 / n
            out["PRECISION_RECALL_MIN_DEN"] = hits32 / min(self.n_test, n)
        n_miss = n - n_hit
        if n_miss == 0:
            out["ROC_AUC"] = 1.0
        elif n_hit:
            # misses ranked below hit j (the j-th hit at rank at[j]): the (n-1-at[j]) later entries minus the later hits
            ordered_pairs = int(((n - 1 - at) - (n_hit - 1 - np.arange(n_hit))).sum())
            out["ROC_AUC"] = np.float32(ordered_pairs) / (n_hit * n_miss)
        if n_hit:
            rank = at + 1.0
            out["MRR"] = 1.0 / rank[0]
            out["ARHR"] = float((1.0 / rank).sum())
            precision_at_hit = np.arange(1, n_hit + 1, dtype=np.float32) / rank
            out["MAP"] = precision_at_hit.sum() / min(self.n_test, n)
            dcg = np.sum((np.power(2, gain) - 1) / self._ln_rank[:n], dtype=np.float32)
            if dcg != 0.0:
                out["NDCG"] = dcg / np.sum(self._ideal_terms[:n], dtype=np.float32)
        return out


def rmse_on_test_items(score_row, test_items, test_ratings):
    """Root mean squared error over the test items with a finite score; NaN when there is none."""
    sq = (score_row[test_items] - test_ratings) ** 2
    usable = np.isfinite(sq)
    count = usable.sum()
    return np.sqrt(np.sum(sq[usable]) / count) if count else np.nan


def _finish(sums, n_eval, cutoffs, names=_SUMMED):
    """Means over the evaluated users + F1 of the mean precision / recall (0 when both are 0)."""
    results = {}
    for c in cutoffs:
        r = {name: sums[c][name] / n_eval for name in names}
        p, rc = r["PRECISION"], r["RECALL"]
        r["F1"] = 2 * (p * rc) / (p + rc) if p + rc != 0 else 0.0
        results[c] = r
    return results


def _pad_lists(lists, K, dtype=np.int64):
    """ragged ranked lists as an [n, K] array, -1 where a list is shorter than K"""
    out = np.full((len(lists), K), -1, dtype=dtype)
    for i, row in enumerate(lists):
        out[i, :len(row)] = row
    return out


def _add_parts(a, b):
    """the results of two consecutive user blocks of a device route as one: sums are added; of the groups route's (sums, sizes,
    per-user values or None) the per-user values of the later block follow those of the earlier one"""
    if isinstance(a, tuple):
        return a[0] + b[0], a[1] + b[1], None if a[2] is None else np.concatenate([a[2], b[2]])
    return a + b


class EvaluatorHoldout(object):
    EVALUATOR_NAME = "EvaluatorHoldout"

    def __init__(self, URM_test_list, cutoff_list, minRatingsPerUser=1, exclude_seen=True, full_metrics=False, diversity_object=None,
                 ignore_items=None, ignore_users=None):
        if isinstance(URM_test_list, list):
            raise ValueError("List of URM_test not supported")
        self.cutoff_list = list(cutoff_list)
        self.max_cutoff = max(self.cutoff_list)
        self.minRatingsPerUser = minRatingsPerUser
        self.exclude_seen = exclude_seen
        self.full_metrics = bool(full_metrics)
        self.URM_test = sps.csr_matrix(URM_test_list)
        self.n_users, self.n_items = self.URM_test.shape
        n_ratings = np.ediff1d(self.URM_test.indptr)
        users = np.arange(self.n_users)[n_ratings >= minRatingsPerUser]
        self.ignore_items_flag = ignore_items is not None
        self.ignore_items_ID = np.array([] if ignore_items is None else ignore_items, dtype=np.int64).reshape(-1)
        self.ignore_users_ID = np.array([] if ignore_users is None else ignore_users, dtype=np.int64).reshape(-1)
        if ignore_users is not None:
            users = users[~np.isin(users, self.ignore_users_ID)]       # ascending (the reference's set difference has no order)
        self.usersToEvaluate = list(users)
        # what the hooks of a device route and `recommend_topk` / `recommend_candidates` get on top of their old arguments
        self._ignore_kw = {"remove_CustomItems_flag": True} if self.ignore_items_flag else {}
        self.diversity_object = diversity_object
        self._diversity = None          # the item diversity matrix every route uses: float32, rounded once
        if diversity_object is not None:
            D = np.asarray(getattr(diversity_object, "item_diversity_matrix", diversity_object))
            if D.shape != (self.n_items, self.n_items):
                raise ValueError("diversity_object: a %d x %d item diversity matrix, given %r" % (self.n_items, self.n_items, D.shape))
            assert np.all(D >= 0.0) and np.all(D <= 1.0), "item_diversity_matrix contains value greater than 1.0 or lower than 0.0"
            self._diversity = np.ascontiguousarray(D, dtype=np.float32)

    def _new_sums(self):
        names = _SUMMED + ((DIVERSITY,) if self._diversity is not None else ())
        return {c: dict.fromkeys(names, 0.0) for c in self.cutoff_list}

    def get_user_relevant_items(self, user_id):
        return self.URM_test.indices[self.URM_test.indptr[user_id]:self.URM_test.indptr[user_id + 1]]

    def get_user_test_ratings(self, user_id):
        return self.URM_test.data[self.URM_test.indptr[user_id]:self.URM_test.indptr[user_id + 1]]

    def _recommend(self, rec, users, return_scores, items_to_compute=None):
        """the one `recommend` call of every host route (the keyword set of Evaluator.py:264-270)"""
        restrict = {} if items_to_compute is None else {"items_to_compute": items_to_compute}
        return rec.recommend(users, remove_seen_flag=self.exclude_seen, cutoff=self.max_cutoff, remove_top_pop_flag=False,
                             remove_CustomItems_flag=self.ignore_items_flag, return_scores=return_scores, **restrict)

    def _ignoring_items(self, call, recommender_object):
        """`call(recommender_object)` between set_items_to_ignore(ignore_items) and reset_items_to_ignore() (Evaluator.py:369-370,
        410-411); the reset runs even when the recommender raises"""
        if not self.ignore_items_flag:
            return call(recommender_object)
        recommender_object.set_items_to_ignore(self.ignore_items_ID)
        try:
            return call(recommender_object)
        finally:
            recommender_object.reset_items_to_ignore()

    def evaluateRecommender(self, recommender_object):
        """(results[cutoff][metric], text) of the class's protocol (`_evaluate`), the recommender ignoring `ignore_items` for the
        duration."""
        return self._ignoring_items(self._evaluate, recommender_object)

    def _evaluate(self, recommender_object):
        """Users are scored in blocks of min(1000, 1e8/n_items) through `recommender.recommend(..., return_scores=True)`
        (Evaluator.py:237-277)."""
        block_size = min(1000, int(1e8 / self.n_items))
        sums = self._new_sums()
        full = _FullSums(self.cutoff_list, self.n_items) if self.full_metrics else None
        w_novelty = w_popularity = None
        if full is not None:
            w_novelty, w_popularity = popularity_weights(item_popularity(_train_matrix(recommender_object)))
        users = np.asarray(self.usersToEvaluate, dtype=np.int64)
        for lo in range(0, len(users), max(block_size, 1)):
            batch = users[lo:lo + block_size]
            rec_lists, scores_batch = self._recommend(recommender_object, batch, True)
            assert len(rec_lists) == len(batch) and scores_batch.shape == (len(batch), self.n_items)
            for user, recommended, score_row in zip(batch, rec_lists, scores_batch):
                self._add_user(sums, full, user, recommended, score_row, w_novelty, w_popularity)
        return self._finish_results(sums, full, len(users))

    # ---- metrics per group of users ----------------------------------------------------------------------------------------
    def evaluateRecommenderByGroup(self, recommender_object, user_groups, return_per_user=False):
        """The accuracy metrics per group of users instead of over all of them (what the reference's user-activity study,
        MFLearned.py:80-145, computes for MAP; also metrics per segment or fold, and per-user values for a significance test).
        `user_groups`: one integer per row of URM_test, the user's group; -1 = in no group.  Users below minRatingsPerUser
        are not evaluated whatever their group (`usersToEvaluate`, as in evaluateRecommender).
        Returns {group: {cutoff: {metric: value}, "n_users": n}} for every group value >= 0 of `user_groups`: the nine values
        of ganmf_amd._lib.EVAL_METRICS as means over the group's n evaluated users, and F1 from the group's mean precision
        and recall as evaluateRecommender forms it; a group without evaluated users gets zeros.  RMSE and the
        beyond-accuracy metrics are NOT part of the grouped row (`full_metrics` is ignored): RMSE needs every score, the
        others are properties of a whole set of lists.  Per-user values are float64 (RankedListMetrics(dtype=np.float64)) on
        every class and route.  `return_per_user=True`: (that dict, the [n_evaluated, n_cutoffs, 9] per-user values, the
        evaluated user ids in the same order).  `ignore_items` / `ignore_users` apply as in evaluateRecommender; the diversity is not
        part of the grouped row."""
        return self._ignoring_items(lambda rec: self._evaluate_by_group(rec, user_groups, return_per_user), recommender_object)

    def _evaluate_by_group(self, recommender_object, user_groups, return_per_user):
        labels, group_idx = self._group_index(user_groups)
        return self._finish_groups(labels, group_idx, self._per_user_host(recommender_object), return_per_user)

    def _group_index(self, user_groups):
        """(the group values >= 0 in ascending order, the index into them of every evaluated user or -1)"""
        groups = np.asarray(user_groups).reshape(-1)
        if groups.shape[0] != self.n_users or not np.issubdtype(groups.dtype, np.integer) or (len(groups) and groups.min() < -1):
            raise ValueError("user_groups: one integer >= -1 per row of URM_test")
        labels = np.unique(groups[groups >= 0])
        of_eval = groups[np.asarray(self.usersToEvaluate, dtype=np.int64)]
        return labels, np.where(of_eval >= 0, np.searchsorted(labels, of_eval), -1).astype(np.int64)

    def _ranked_lists(self, recommender_object):
        """the evaluated users' ranked lists in the order of usersToEvaluate, from the calls evaluateRecommender makes"""
        block_size = max(min(1000, int(1e8 / self.n_items)), 1)
        users = np.asarray(self.usersToEvaluate, dtype=np.int64)
        for lo in range(0, len(users), block_size):
            batch = users[lo:lo + block_size]
            rec_lists, _ = self._recommend(recommender_object, batch, True)
            assert len(rec_lists) == len(batch)
            for recommended in rec_lists:
                yield recommended

    def _per_user_host(self, recommender_object):
        """[n_evaluated, n_cutoffs, 9] float64: every evaluated user's values in the order of ganmf_amd._lib.EVAL_METRICS"""
        from ._lib import EVAL_METRICS
        users = self.usersToEvaluate
        vals = np.zeros((len(users), len(self.cutoff_list), len(EVAL_METRICS)), dtype=np.float64)
        for i, recommended in enumerate(self._ranked_lists(recommender_object)):
            user = users[i]
            scorer = RankedListMetrics(self.get_user_relevant_items(user), self.get_user_test_ratings(user), self.max_cutoff,
                                       dtype=np.float64)
            hit, gain = scorer.match(np.asarray(recommended))
            for ci, c in enumerate(self.cutoff_list):
                row = scorer(hit, gain, c)
                vals[i, ci] = [row[name] for name in EVAL_METRICS]
        return vals

    def _finish_groups(self, labels, group_idx, per_user, return_per_user, sums=None, sizes=None):
        """the result of evaluateRecommenderByGroup from the per-user values, or from group sums / sizes formed elsewhere"""
        from ._lib import EVAL_METRICS
        if sums is None:
            sums = np.zeros((len(labels), len(self.cutoff_list), len(EVAL_METRICS)), dtype=np.float64)
            sizes = np.zeros(len(labels), dtype=np.int64)
            for g in range(len(labels)):
                member = group_idx == g
                sizes[g] = int(member.sum())
                sums[g] = per_user[member].sum(axis=0)
        results = {}
        for g, label in enumerate(labels):
            n = int(sizes[g])
            if n:
                rows = _finish({c: dict(zip(EVAL_METRICS, sums[g, ci])) for ci, c in enumerate(self.cutoff_list)}, n,
                               self.cutoff_list, names=EVAL_METRICS)
                rows = {c: {m: float(v) for m, v in row.items()} for c, row in rows.items()}
            else:
                rows = {c: dict.fromkeys(EVAL_METRICS + ("F1",), 0.0) for c in self.cutoff_list}
            rows["n_users"] = n
            results[int(label)] = rows
        if return_per_user:
            return results, per_user, np.asarray(self.usersToEvaluate, dtype=np.int64)
        return results

    def _add_user(self, sums, full, user, recommended, score_row, w_novelty, w_popularity):
        """one user's ranked list and score row into the running sums of every cut-off (Evaluator.py:280-335)"""
        test_items, test_ratings = self.get_user_relevant_items(user), self.get_user_test_ratings(user)
        scorer = RankedListMetrics(test_items, test_ratings, self.max_cutoff)
        hit, gain = scorer.match(recommended)
        user_rmse = rmse_on_test_items(score_row, test_items, test_ratings)
        for c in self.cutoff_list:
            acc = sums[c]
            for name, value in scorer(hit, gain, c).items():
                acc[name] += value
            acc["RMSE"] += user_rmse
            if self._diversity is not None:
                acc[DIVERSITY] += list_diversity(self._diversity, np.asarray(recommended[:c], dtype=np.int64).reshape(1, -1), [c])[0, 0]
            if full is not None:
                listed = np.asarray(recommended[:c], dtype=np.int64)
                if len(listed) > 0:
                    full.counts[c][listed] += 1
                    full.novelty[c] += np.sum(w_novelty[listed])
                    full.popularity[c] += np.sum(w_popularity[listed]) / len(listed)
                    full.nonempty[c] += 1

    def _finish_results(self, sums, full, n_eval, rmse=True, as_float=False):
        """(results, text) from the running sums.  rmse=False: the route did not compute it, NaN.  as_float: Python floats (the
        reference-order classes return the float32 / float64 scalars their sums are made of)."""
        diversity = self._diversity is not None
        if n_eval == 0:
            print("WARNING: No users had a sufficient number of relevant items")
            results = {c: dict.fromkeys(METRICS + ((DIVERSITY,) if diversity else ()), 0.0) for c in self.cutoff_list}
        else:
            results = _finish(sums, n_eval, self.cutoff_list)
            for c in self.cutoff_list:
                if as_float:
                    results[c] = {m: float(v) for m, v in results[c].items()}
                if not rmse:
                    results[c]["RMSE"] = float("nan")
                if diversity:
                    results[c][DIVERSITY] = float(sums[c][DIVERSITY]) / n_eval
        if full is not None:
            results = full.rows(results, n_eval, self.cutoff_list, self.n_items, self.n_users, self.ignore_items_ID, self.ignore_users_ID)
        return results, get_result_string(results)


_DEVICE_TOKENS = itertools.count(1)


class EvaluatorHoldoutFast(EvaluatorHoldout):
    """Same protocol and result dictionaries as EvaluatorHoldout (Evaluator.py:214-414), but consumes only the
    top-`max_cutoff` ids of each user — `recommender.recommend_topk(...)` when the recommender has it (device
    selection, include/ganmf_hip.h: ganmf_recommend), else `recommend(..., return_scores=False)` — and computes
    the ranking metrics for a whole block of users at once.  Sums are float64 (the per-user functions above
    follow the reference's float32 sums); the two agree to ~1e-6 relative.  RMSE needs every score and is reported
    as NaN here unless `full_metrics=True`: then the device route forms it inside the selection
    kernel (ganmf_evaluate_full) and the host route takes ids and scores from `recommend(..., return_scores=True)`."""
    EVALUATOR_NAME = "EvaluatorHoldoutFast"

    def __init__(self, URM_test_list, cutoff_list, minRatingsPerUser=1, exclude_seen=True, full_metrics=False, diversity_object=None,
                 ignore_items=None, ignore_users=None):
        super().__init__(URM_test_list, cutoff_list, minRatingsPerUser=minRatingsPerUser, exclude_seen=exclude_seen,
                         full_metrics=full_metrics, diversity_object=diversity_object, ignore_items=ignore_items,
                         ignore_users=ignore_users)
        K = self.max_cutoff
        self._users = np.asarray(self.usersToEvaluate, dtype=np.int64)
        self._n_test = np.ediff1d(self.URM_test.indptr)[self._users].astype(np.int64)
        # relevance lookup: stored entries of URM_test are the relevant items (Evaluator.py:46-52), value = gain
        self._rel = sps.csr_matrix((np.ones_like(self.URM_test.data, dtype=np.float64), self.URM_test.indices,
                                    self.URM_test.indptr), shape=self.URM_test.shape)
        self._gain = sps.csr_matrix((np.power(2.0, self.URM_test.data.astype(np.float32)).astype(np.float64) - 1.0,
                                     self.URM_test.indices, self.URM_test.indptr), shape=self.URM_test.shape)
        # ideal DCG prefix sums: ratings sorted descending, first K, discounted (metrics.py ndcg/dcg)
        disc = 1.0 / np.log(np.arange(K, dtype=np.float32) + 2).astype(np.float64)
        ideal = np.zeros((len(self._users), K))
        for i, u in enumerate(self._users):
            r = np.sort(self.get_user_test_ratings(u))[::-1][:K].astype(np.float32)
            ideal[i, :len(r)] = (np.power(2.0, r).astype(np.float64) - 1.0) * disc[:len(r)]
        self._ideal_cum = np.cumsum(ideal, axis=1)
        self._disc = disc
        # device route (recommender.evaluate_on_device -> ganmf_evaluate): the test matrix with sorted rows and its DCG gains
        self._test_sorted = self.URM_test.tocsr().copy()
        self._test_sorted.sort_indices()
        self._test_gain = np.power(2.0, self._test_sorted.data.astype(np.float32)).astype(np.float64) - 1.0
        self._test_rating = np.ascontiguousarray(self._test_sorted.data, dtype=np.float32)    # RMSE on the device (full_metrics)
        self.use_device_metrics = True
        # users per call of every route; None: the defaults of evaluateRecommender (tests force several blocks)
        self._block_size = None
        # identifies THIS evaluator's test matrix on the device (never reused, unlike id(): CPython hands the id of a freed
        # evaluator to the next one, and a recommender keyed on it would score the new evaluator against the old test matrix)
        self._device_token = next(_DEVICE_TOKENS)

    # ---- users per call of every route: `_block_size` when set, else the route's own rule ---------------------------------------
    def _host_block(self):
        return self._block_size or max(1, min(4096, int(1e8 / self.n_items)))

    def _device_block(self):
        """the device forms a [block, n_items] score matrix (+ block x K doubles) per call: the cap of the host routes, unclipped"""
        return self._block_size or max(1, int(1e8 / self.n_items))

    def _topk(self, rec, batch):
        if hasattr(rec, "recommend_topk"):
            return np.asarray(rec.recommend_topk(batch, self.max_cutoff, remove_seen_flag=self.exclude_seen, **self._ignore_kw))
        return _pad_lists(self._recommend(rec, batch, False), self.max_cutoff)

    def _topk_and_rmse(self, rec, batch):
        """full_metrics host route: the ids of recommend(..., return_scores=True) and the sum of the users' RMSE"""
        lists, scores = self._recommend(rec, batch, True)
        rmse_sum = 0.0
        for i, u in enumerate(batch):
            rmse_sum += rmse_on_test_items(scores[i], self.get_user_relevant_items(u), self.get_user_test_ratings(u))
        return _pad_lists(lists, self.max_cutoff), rmse_sum

    def _device_route(self, rec, hook):
        """whether the device route through `rec.<hook>` is open: asked for, somebody to evaluate, and the recommender has it"""
        return self.use_device_metrics and len(self._users) > 0 and hasattr(rec, hook)

    def _device_blocks(self, call, n, block):
        """The one loop of every device route: `call(slice)` over the n evaluated users in blocks of `block`, the parts added in
        block order (_add_parts).  None -- the caller then takes its host route for ALL users -- as soon as a block returns None
        (the recommender declines) or the device runs out of memory."""
        total = None
        try:
            for start in range(0, n, block):
                part = call(slice(start, min(start + block, n)))
                if part is None:
                    return None
                total = part if total is None else _add_parts(total, part)
        except MemoryError:
            return None
        return total

    def _device_sums(self, rec, call, block, candidates=None):
        """A device route over all user blocks, finished: (results, text), or None when the host route is to be taken.
        `call(slice, ratings, item_weights, counts)` returns one block's sums from the recommender's hook: nine per cut-off
        (the three arguments None), or with full_metrics 13 per cut-off, the block's per-item counts added into `counts`.
        With a diversity_object one more call per block, `rec.evaluate_diversity_on_device` (the same ranking; `candidates`: every
        user among its own), whose sums become one more column; a recommender without that hook takes the host route."""
        diversity = self._diversity is not None
        if diversity and not hasattr(rec, "evaluate_diversity_on_device"):
            return None
        full = _FullSums(self.cutoff_list, self.n_items) if self.full_metrics else None
        ratings = weights = counts = None
        if full is not None:
            ratings, weights = self._test_rating, popularity_weights(item_popularity(_train_matrix(rec)))
            counts = np.zeros((len(self.cutoff_list), self.n_items), dtype=np.int64)

        def block_sums(sl):
            part = call(sl, ratings, weights, counts)
            if part is None or not diversity:
                return part
            div = rec.evaluate_diversity_on_device(self._device_token, self._diversity, self._users[sl], self.cutoff_list,
                                                   remove_seen_flag=self.exclude_seen, candidates_csr=candidates, **self._ignore_kw)
            return None if div is None else np.concatenate([part, np.asarray(div, dtype=np.float64).reshape(-1, 1)], axis=1)
        dev = self._device_blocks(block_sums, len(self._users), block)
        return None if dev is None else self._from_device(dev, full, counts)

    def _evaluate(self, recommender_object):
        rec = recommender_object
        if self._device_route(rec, "evaluate_full_on_device" if self.full_metrics else "evaluate_on_device"):
            # everything on the device: scores, seen mask, top-k AND the metric sums (only the sums, and the counts of a full row,
            # come back), added up over the user blocks
            def call(sl, ratings, weights, counts):
                if self.full_metrics:
                    return rec.evaluate_full_on_device(self._device_token, self._test_sorted, self._test_gain, ratings, weights,
                                                       self._users[sl], self.cutoff_list, self._disc, self._ideal_cum[sl],
                                                       remove_seen_flag=self.exclude_seen, counts=counts, **self._ignore_kw)
                return rec.evaluate_on_device(self._device_token, self._test_sorted, self._test_gain, self._users[sl],
                                              self.cutoff_list, self._disc, self._ideal_cum[sl], remove_seen_flag=self.exclude_seen,
                                              **self._ignore_kw)
            got = self._device_sums(rec, call, self._device_block())
            if got is not None:
                return got
        n_eval = len(self._users)
        sums = self._new_sums()
        full = _FullSums(self.cutoff_list, self.n_items) if self.full_metrics else None
        w_novelty = w_popularity = None
        if full is not None:
            w_novelty, w_popularity = popularity_weights(item_popularity(_train_matrix(rec)))
        block_size = self._host_block()
        for start in range(0, n_eval, block_size):
            sl = slice(start, min(start + block_size, n_eval))
            rmse_sum = 0.0
            if full is not None:
                items, rmse_sum = self._topk_and_rmse(rec, self._users[sl])
            else:
                items = self._topk(rec, self._users[sl])
            self._add_block(sums, full, items, sl, rmse_sum, w_novelty, w_popularity)
        return self._finish_results(sums, full, n_eval, rmse=full is not None, as_float=True)

    def _ranked_lists(self, recommender_object):
        """the host route's lists: `_topk` in the blocks of evaluateRecommender"""
        block_size = self._host_block()
        for start in range(0, len(self._users), block_size):
            for row in self._topk(recommender_object, self._users[start:start + block_size]):
                yield row[row >= 0]

    def _device_groups(self, rec, labels, group_idx, per_user, block, candidates=None):
        """(sums [G, C, 9], sizes [G], per-user values or None) of evaluate_groups_on_device over all user blocks, added in block
        order; None when the recommender declines the device route or the device runs out of memory"""
        return self._device_blocks(
            lambda sl: rec.evaluate_groups_on_device(self._device_token, self._test_sorted, self._test_gain, self._users[sl],
                                                     self.cutoff_list, self._disc, self._ideal_cum[sl], group_idx[sl], len(labels),
                                                     remove_seen_flag=self.exclude_seen, candidates_csr=candidates, per_user=per_user,
                                                     **self._ignore_kw),
            len(self._users), block)

    def _evaluate_by_group(self, recommender_object, user_groups, return_per_user):
        """EvaluatorHoldout.evaluateRecommenderByGroup; with a recommender that has `evaluate_groups_on_device`
        (ganmf_evaluate_groups) ranking, per-user values and group sums stay on the device, and the host route is taken exactly
        where evaluateRecommender takes it."""
        labels, group_idx = self._group_index(user_groups)
        if self._device_route(recommender_object, "evaluate_groups_on_device"):
            got = self._device_groups(recommender_object, labels, group_idx, return_per_user, self._device_block())
            if got is not None:
                return self._finish_groups(labels, group_idx, got[2], return_per_user, sums=got[0], sizes=got[1])
        return self._finish_groups(labels, group_idx, self._per_user_host(recommender_object), return_per_user)

    def _from_device(self, dev, full, counts):
        """(results, text) from a device route's sums over all evaluated users: [n_cutoffs, 9] in the order of EVAL_METRICS (RMSE is
        not computed there), or with `full` [n_cutoffs, 13] in the order of EVAL_FULL_METRICS beside the [n_cutoffs, n_items] counts"""
        from ._lib import EVAL_FULL_METRICS, EVAL_METRICS
        col = {name: i for i, name in enumerate(EVAL_METRICS if full is None else EVAL_FULL_METRICS)}
        sums = self._new_sums()
        for ci, c in enumerate(self.cutoff_list):
            if self._diversity is not None:             # the column _device_sums appended
                sums[c][DIVERSITY] = float(dev[ci, len(col)])
            for name in _SUMMED:
                if name in col:
                    sums[c][name] = float(dev[ci, col[name]])
            if full is not None:
                full.counts[c] = counts[ci]
                full.novelty[c] = float(dev[ci, col["NOVELTY"]])
                full.popularity[c] = float(dev[ci, col["AVERAGE_POPULARITY"]])
                full.nonempty[c] = int(round(dev[ci, col["NON_EMPTY"]]))
        return self._finish_results(sums, full, len(self._users), rmse=full is not None, as_float=True)

    def _add_block(self, sums, full, items, sl, rmse_sum, w_novelty, w_popularity):
        """the ranked ids [len(block), K] (-1 padded) of the users self._users[sl] into the float64 sums of every cut-off"""
        K = self.max_cutoff
        batch = self._users[sl]
        inv_rank = 1.0 / np.arange(1, K + 1, dtype=np.float64)
        assert items.shape == (len(batch), K)
        valid = items >= 0
        safe = np.where(valid, items, 0)
        rows = np.repeat(np.arange(len(batch)), K)
        rel_block, gain_block = self._rel[batch], self._gain[batch]
        is_rel = np.asarray(rel_block[rows, safe.ravel()]).reshape(len(batch), K) > 0
        is_rel &= valid
        gain = np.asarray(gain_block[rows, safe.ravel()]).reshape(len(batch), K) * is_rel
        n_test = self._n_test[sl].astype(np.float64)
        length = valid.sum(axis=1)
        diversity = None if self._diversity is None else list_diversity(self._diversity, items, self.cutoff_list)
        for ci, c in enumerate(self.cutoff_list):
            r = sums[c]
            if diversity is not None:
                r[DIVERSITY] += diversity[:, ci].sum()
            rel = is_rel[:, :c].astype(np.float64)
            neg = (valid[:, :c] & ~is_rel[:, :c]).astype(np.float64)
            len_c = np.minimum(length, c).astype(np.float64)
            hits = rel.sum(axis=1)
            nneg = neg.sum(axis=1)
            # AUC over the list: for each hit, the negatives ranked after it (metrics.py roc_auc)
            neg_after = nneg[:, None] - np.cumsum(neg, axis=1)
            pairs = (rel * neg_after).sum(axis=1)
            auc = np.where(nneg == 0, 1.0, np.where(hits > 0, pairs / np.maximum(hits * nneg, 1.0), 0.0))
            nz = np.maximum(len_c, 1.0)
            r["ROC_AUC"] += auc.sum()
            r["PRECISION"] += np.where(len_c > 0, hits / nz, 0.0).sum()
            r["PRECISION_RECALL_MIN_DEN"] += np.where(len_c > 0, hits / np.maximum(np.minimum(n_test, len_c), 1.0), 0.0).sum()
            r["RECALL"] += (hits / n_test).sum()
            dcg_rank = (gain[:, :c] * self._disc[:c]).sum(axis=1)
            li = np.maximum(len_c.astype(np.int64) - 1, 0)
            ideal = self._ideal_cum[sl][np.arange(len(batch)), li]
            r["NDCG"] += np.where(dcg_rank > 0, dcg_rank / np.where(ideal > 0, ideal, 1.0), 0.0).sum()
            r["HIT_RATE"] += hits.sum()
            r["ARHR"] += (rel * inv_rank[:c]).sum()
            first = np.argmax(rel > 0, axis=1)
            r["MRR"] += np.where(hits > 0, inv_rank[first], 0.0).sum()
            p_at_k = rel * np.cumsum(rel, axis=1) * inv_rank[:c]
            r["MAP"] += np.where(len_c > 0, p_at_k.sum(axis=1) / np.maximum(np.minimum(n_test, len_c), 1.0), 0.0).sum()
            if full is not None:
                r["RMSE"] += rmse_sum
                listed = valid[:, :c]
                full.counts[c] += np.bincount(items[:, :c][listed], minlength=self.n_items)
                full.novelty[c] += (w_novelty[safe[:, :c]] * listed).sum()
                pop_sum = (w_popularity[safe[:, :c]] * listed).sum(axis=1)
                full.popularity[c] += np.where(len_c > 0, pop_sum / nz, 0.0).sum()
                full.nonempty[c] += int((len_c > 0).sum())


def items_to_rank(URM_test, URM_test_negative):
    """URM_items_to_rank of the reference (Evaluator.py:450-452): test items + negative items of every user, binarised, an item
    stored in both matrices kept once, explicit zeros dropped; rows sorted."""
    m = sps.csr_matrix(sps.csr_matrix(URM_test).astype(bool)) + sps.csr_matrix(sps.csr_matrix(URM_test_negative).astype(bool))
    m = sps.csr_matrix(m)
    m.eliminate_zeros()
    m.sort_indices()
    m.data = np.ones_like(m.data)
    return m


class _NegativeSample(object):
    """What the two negative-sample evaluators add to their hold-out base: every user's candidates, `URM_items_to_rank`"""

    def __init__(self, URM_test_list, URM_test_negative, cutoff_list, minRatingsPerUser=1, exclude_seen=True, full_metrics=False,
                 diversity_object=None, ignore_items=None, ignore_users=None):
        super().__init__(URM_test_list, cutoff_list, minRatingsPerUser=minRatingsPerUser, exclude_seen=exclude_seen,
                         full_metrics=full_metrics, diversity_object=diversity_object, ignore_items=ignore_items,
                         ignore_users=ignore_users)
        self.URM_items_to_rank = items_to_rank(self.URM_test, URM_test_negative)
        if self.URM_items_to_rank.shape != self.URM_test.shape:
            raise ValueError("URM_test_negative must have the shape of URM_test")

    def _get_user_specific_items_to_compute(self, user_id):
        m = self.URM_items_to_rank
        return m.indices[m.indptr[user_id]:m.indptr[user_id + 1]]

    def _recommend_user(self, rec, user, return_scores):
        """the reference's one call per user: recommend(user, items_to_compute=the user's candidates)"""
        return self._recommend(rec, np.atleast_1d(user), return_scores, self._get_user_specific_items_to_compute(user))


class EvaluatorNegativeItemSample(_NegativeSample, EvaluatorHoldout):
    """The reference's negative-sample protocol (Evaluator.py:419-590) in its own order: every evaluated user's test items are
    ranked only against that user's candidates `URM_items_to_rank` = URM_test + URM_test_negative ("leave-one-out + N sampled
    negatives"), through ONE `recommend(user, items_to_compute=candidates, return_scores=True)` call per user, with the
    reference's float32 per-user sums.

    What "only against the candidates" means is the recommender's business, as in the reference: a recommender that honours
    `items_to_compute` (the MF contract, Base/BaseMatrixFactorizationRecommender.py:113-119; GANMF(score_contract="mf")) scores
    every other item -inf; the reference's own GANMF ignores `items_to_compute` (GANMF.py:285-292; the default
    score_contract="ganmf" here), and this evaluator around it ranks the whole catalogue, exactly as the reference's does.

    `ignore_items` applies to EVERY user.  The reference calls reset_items_to_ignore() inside its user loop (Evaluator.py:530), so
    there only the first evaluated user is filtered -- a quirk this class (and the Fast one) deliberately does not copy."""
    EVALUATOR_NAME = "EvaluatorNegativeItemSample"

    def _evaluate(self, recommender_object):
        sums = self._new_sums()
        full = _FullSums(self.cutoff_list, self.n_items) if self.full_metrics else None
        w_novelty = w_popularity = None
        if full is not None:
            w_novelty, w_popularity = popularity_weights(item_popularity(_train_matrix(recommender_object)))
        for user in self.usersToEvaluate:
            rec_lists, scores = self._recommend_user(recommender_object, user, True)
            assert len(rec_lists) == 1 and scores.shape == (1, self.n_items)
            self._add_user(sums, full, user, rec_lists[0], scores[0], w_novelty, w_popularity)
        return self._finish_results(sums, full, len(self.usersToEvaluate))

    def _ranked_lists(self, recommender_object):
        for user in self.usersToEvaluate:
            rec_lists, _ = self._recommend_user(recommender_object, user, True)
            assert len(rec_lists) == 1
            yield rec_lists[0]


class EvaluatorNegativeItemSampleFast(_NegativeSample, EvaluatorHoldoutFast):
    """EvaluatorNegativeItemSample's protocol and result dictionaries, consuming only the top-`max_cutoff` ids of every user, with
    the float64 sums and the finishing code of EvaluatorHoldoutFast.  Routes, in this order:

      device   `recommender.evaluate_candidates_on_device(...)` (ganmf_evaluate_candidates: candidate scoring, masks, top-k and the
               metric sums in HIP kernels; only the sums, and the counts of a full row, come back), in user blocks;
      blocks   `recommender.recommend_candidates(users, candidates, cutoff, ...)` -> [n, cutoff] ids (ganmf_recommend_candidates),
               metrics on the host (nine-metric rows: RMSE, which needs the scores, is NaN as in EvaluatorHoldoutFast); a
               ValueError / RuntimeError from it (limits of the block-wise API) sends the remaining blocks to the next route;
      users    one `recommend(user, items_to_compute=candidates, ...)` per user, as the reference-order class calls it.

    Contracts.  The result is what EvaluatorNegativeItemSample returns for the same recommender.  A recommender that ignores
    `items_to_compute` -- the reference's GANMF (GANMF.py:285-292) and GANMF here under the default score_contract="ganmf" --
    is ranked over the whole catalogue by the reference's evaluator; such a recommender says so (`honours_items_to_compute` is
    False), declines the device route (None), and this class then evaluates it exactly as EvaluatorHoldoutFast does (full-width
    routes).  Under score_contract="mf" the candidate kernel is used."""
    EVALUATOR_NAME = "EvaluatorNegativeItemSampleFast"

    # ---- users per call of the candidate routes (the device route holds block x K doubles and two ints per candidate, no score
    # matrix) ------------------------------------------------------------------------------------------------------------------
    def _candidate_host_block(self):
        return self._block_size or 4096

    def _candidate_device_block(self):
        return self._block_size or 65536

    def _per_user(self, rec, batch, with_scores):
        """ids [len(batch), K] (-1 padded) from one recommend(user, items_to_compute=...) per user, and the users' RMSE sum"""
        lists = []
        rmse_sum = 0.0
        for u in batch:
            got = self._recommend_user(rec, u, with_scores)
            user_lists, scores = got if with_scores else (got, None)
            lists.append(user_lists[0])
            if with_scores:
                rmse_sum += float(rmse_on_test_items(scores[0], self.get_user_relevant_items(u), self.get_user_test_ratings(u)))
        return _pad_lists(lists, self.max_cutoff), rmse_sum

    def _candidate_blocks(self, rec, with_scores):
        """The host candidate routes: yields (slice of the evaluated users, their ids [len, K] -1 padded, their RMSE sum -- 0
        without scores) block by block.  Blocks go through `rec.recommend_candidates` (ids only: not with_scores) while it takes
        them; its first ValueError / RuntimeError (beyond what the block-wise API takes: a cut-off or a candidate list over its
        limits) sends that block and every later one user by user, as the full row goes."""
        by_block = not with_scores and hasattr(rec, "recommend_candidates")
        n_eval, block_size = len(self._users), self._candidate_host_block()
        for start in range(0, n_eval, block_size):
            sl = slice(start, min(start + block_size, n_eval))
            items, rmse_sum = None, 0.0
            if by_block:
                try:
                    items = np.asarray(rec.recommend_candidates(self._users[sl], self.URM_items_to_rank, self.max_cutoff,
                                                                remove_seen_flag=self.exclude_seen,
                                                                candidates_key=self._device_token, **self._ignore_kw), dtype=np.int64)
                except (ValueError, RuntimeError):
                    by_block = False
            if items is None:
                items, rmse_sum = self._per_user(rec, self._users[sl], with_scores)
            yield sl, items, rmse_sum

    def _ranked_lists(self, recommender_object):
        """the host routes of evaluateRecommender: full width for a recommender that ignores items_to_compute, else the candidate
        blocks"""
        if not getattr(recommender_object, "honours_items_to_compute", True):
            for row in super()._ranked_lists(recommender_object):
                yield row
            return
        for _, items, _ in self._candidate_blocks(recommender_object, False):
            for row in items:
                yield row[row >= 0]

    def _evaluate_by_group(self, recommender_object, user_groups, return_per_user):
        """EvaluatorHoldout.evaluateRecommenderByGroup with every user ranked among its own candidates; the routes of
        evaluateRecommender in its order (device candidates, full width for a recommender that ignores items_to_compute, blocks,
        users)."""
        rec = recommender_object
        labels, group_idx = self._group_index(user_groups)
        if self._device_route(rec, "evaluate_groups_on_device"):
            got = self._device_groups(rec, labels, group_idx, return_per_user, self._candidate_device_block(),
                                      candidates=self.URM_items_to_rank)
            if got is not None:
                return self._finish_groups(labels, group_idx, got[2], return_per_user, sums=got[0], sizes=got[1])
        if not getattr(rec, "honours_items_to_compute", True):
            return super()._evaluate_by_group(rec, user_groups, return_per_user)
        return self._finish_groups(labels, group_idx, self._per_user_host(rec), return_per_user)

    def _evaluate(self, recommender_object):
        rec = recommender_object
        if self._device_route(rec, "evaluate_candidates_on_device"):
            got = self._device_sums(
                rec, lambda sl, ratings, weights, counts: rec.evaluate_candidates_on_device(
                    self._device_token, self._test_sorted, self._test_gain, self.URM_items_to_rank, self._users[sl], self.cutoff_list,
                    self._disc, self._ideal_cum[sl], remove_seen_flag=self.exclude_seen, ratings=ratings, item_weights=weights,
                    counts=counts, **self._ignore_kw),
                self._candidate_device_block(), candidates=self.URM_items_to_rank)
            if got is not None:
                return got
        if not getattr(rec, "honours_items_to_compute", True):
            # the reference's evaluator around this recommender ranks the whole catalogue: the full-width routes
            return super()._evaluate(rec)
        sums = self._new_sums()
        full = _FullSums(self.cutoff_list, self.n_items) if self.full_metrics else None
        w_novelty = w_popularity = None
        if full is not None:
            w_novelty, w_popularity = popularity_weights(item_popularity(_train_matrix(rec)))
        for sl, items, rmse_sum in self._candidate_blocks(rec, with_scores=full is not None):
            self._add_block(sums, full, items, sl, rmse_sum, w_novelty, w_popularity)
        return self._finish_results(sums, full, len(self._users), rmse=full is not None, as_float=True)
