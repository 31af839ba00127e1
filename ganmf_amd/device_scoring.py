"""The device-scoring surface of a factor model: everything a recommender needs to score, recommend and be evaluated without its
scores leaving the device.  The methods need only `self.engine` (ganmf_amd.engine.Engine), `self.mode` ('user' | 'item'),
`self.score_contract` ("ganmf" | "mf"), `self._URM_eval` (users x items), `self.n_users` / `self.n_items`, the ignore-list attributes of
BaseRecommender and a `_require_engine()` that raises while there is no device state.  GANMF / DisGANMF and IALSRecommender inherit
it in front of BaseRecommender, whose host `recommend` is the route of the calls the device selection does not take."""
import collections
import contextlib

import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .evaluation import _pad_lists

# the test matrix an engine holds for device evaluation: the evaluator's token, that engine, whether the ratings went up with it
_TestOnDevice = collections.namedtuple("_TestOnDevice", "key engine has_ratings")


class DeviceScoringMixin(object):

    # under the MF contract a user without a training interaction scores -inf everywhere; a class whose reference scores such a
    # user like any other (the similarity-matrix models: all zeros) sets this to False and keeps the contract's item filter
    mask_cold_users = True

    def _reset_score_filter(self):
        """no item filter; the cold-user mask only under the MF contract (the reference's GANMF scores every user)"""
        self.engine.set_score_filter(None, mask_cold=(self.score_contract == "mf" and self.mask_cold_users))

    # ---- scoring (GANMF.py:285-292) ---------------------------------------------------------------
    def _compute_item_score(self, user_id_array, items_to_compute=None):
        """Scores in evaluation orientation.  score_contract "ganmf" (default; GANMF.py:285-292): U[ids] . V^T for every user,
        `items_to_compute` ignored.  "mf" (BaseMatrixFactorizationRecommender.py:113-119,128-143): `items_to_compute` given ->
        every other item is -inf; users without a training interaction are -inf everywhere; both masks applied on the device."""
        self._require_engine()
        ids = np.asarray(user_id_array).reshape(-1)
        if items_to_compute is None or self.score_contract != "mf":
            return self.engine.scores(ids, transposed=(self.mode == 'item'))
        with self._item_filter(items_to_compute):
            return self.engine.scores(ids, transposed=(self.mode == 'item'))

    def prediction_similarity(self, user_id_array=None, pool=None, return_matrix=False):
        """Cosine similarity of the predictions of `user_id_array` (None: every user) among themselves -- the reference's collapse
        study, AblationStudy.py:88-92,113-117: cosine_similarity(_compute_item_score(all users)), its np.mean and np.std -- formed on
        the device from the unfiltered scores (no score filter under either contract: a -inf has no cosine).  Returns a dict: mean,
        std (population), n, zero_rows; with pool=P also `pooled`, the [P, P] block means behind a heat-map; with
        return_matrix=True also `matrix`, the [n, n] float32 similarities.  No host fallback."""
        self._require_engine()
        ids = np.arange(self.n_users) if user_id_array is None else np.asarray(user_id_array).reshape(-1)
        return self.engine.score_similarity(ids, transposed=(self.mode == 'item'), pool=pool, return_matrix=return_matrix)

    def _item_filter(self, items_to_compute):
        """context (MF contract only): scores / recommend / evaluate restricted to `items_to_compute`; the cold-user mask stays on"""
        eng = self.engine
        reset = self._reset_score_filter
        mask_cold = self.mask_cold_users

        class _Ctx(object):
            def __enter__(self_inner):
                eng.set_score_filter(items_to_compute, mask_cold=mask_cold)

            def __exit__(self_inner, *exc):
                reset()
                return False
        return _Ctx()

    @contextlib.contextmanager
    def _ignored_items(self, remove_CustomItems_flag=False, remove_top_pop_flag=False):
        """context: the union of `items_to_ignore_ID` and `filterTopPop_ItemsID`, each under its flag, is the engine's ignore list
        (ganmf_set_items_to_ignore: -inf in everything that ranks, Base/BaseRecommender.py:80-86, 207-211) for the duration, and
        cleared afterwards; nothing is set for an empty union"""
        parts = []
        if remove_CustomItems_flag:
            parts.append(np.asarray(self.items_to_ignore_ID, dtype=np.int64).reshape(-1))
        if remove_top_pop_flag:
            parts.append(np.asarray(self.filterTopPop_ItemsID, dtype=np.int64).reshape(-1))
        items = np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)
        if len(items) == 0:
            yield
            return
        self.engine.set_items_to_ignore(items)
        try:
            yield
        finally:
            self.engine.set_items_to_ignore(None)

    # ---- recommend (Base/BaseRecommender.py:155-247) ---------------------------------------------
    _DEVICE_TOPK_MAX = 256   # above this the k-round device selection loses to numpy's argpartition

    def recommend_topk(self, user_id_array, cutoff, remove_seen_flag=True, items_to_compute=None, remove_CustomItems_flag=False,
                       remove_top_pop_flag=False):
        """Top-`cutoff` item ids per user as an [n, cutoff] int32 array, -1 padded where a user has fewer
        finite scores; scores, seen-item mask, the two remove_* filters and selection all stay on the device (ganmf_recommend).
        Cut-offs the device selection does not take (above _DEVICE_TOPK_MAX or above the item count) are ranked by
        the host route and padded the same way."""
        self._require_engine()
        ids = np.atleast_1d(np.asarray(user_id_array)).reshape(-1)
        if 1 <= cutoff <= min(self._DEVICE_TOPK_MAX, self.n_items):
            with self._ignored_items(remove_CustomItems_flag, remove_top_pop_flag):
                if items_to_compute is None or self.score_contract != "mf":
                    items, _ = self.engine.recommend(ids, cutoff, transposed=(self.mode == 'item'), remove_seen=remove_seen_flag)
                else:
                    with self._item_filter(items_to_compute):
                        items, _ = self.engine.recommend(ids, cutoff, transposed=(self.mode == 'item'), remove_seen=remove_seen_flag)
            return items
        lists = self.recommend(ids, cutoff=cutoff, remove_seen_flag=remove_seen_flag, items_to_compute=items_to_compute,
                               remove_top_pop_flag=remove_top_pop_flag, remove_CustomItems_flag=remove_CustomItems_flag,
                               return_scores=True)[0]
        return _pad_lists(lists, cutoff, dtype=np.int32)

    def _device_ranking_args(self, user_id_array, cutoffs, max_cutoff, candidates_csr=None):
        """(ids, cutoffs) as the engine's ranking entries take them, or None where the device route does not apply: too many
        cut-offs, one outside [1, min(max_cutoff, n_items)], and with `candidates_csr` also score_contract != "mf" or a requested
        user with more than _lib.CANDIDATES_MAX_PER_ROW candidates"""
        self._require_engine()
        cand = candidates_csr is not None
        if cand and self.score_contract != "mf":
            return None
        cutoffs = list(cutoffs)
        if not cutoffs or len(cutoffs) > L.EVAL_MAX_CUTOFFS or min(cutoffs) < 1 or max(cutoffs) > min(max_cutoff, self.n_items):
            return None
        ids = np.asarray(user_id_array).reshape(-1)
        if cand and len(ids) and np.ediff1d(candidates_csr.indptr)[ids].max() > L.CANDIDATES_MAX_PER_ROW:
            return None
        return ids, cutoffs

    def _prepare_device_evaluation(self, evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, max_cutoff, ratings=None,
                                   item_weights=None, candidates_csr=None):
        """What the four evaluate_*_on_device share.  None: the device route does not apply -- too many cut-offs, one outside
        [1, min(max_cutoff, n_items)], and with `candidates_csr` also score_contract != "mf" or a requested user with more than
        _lib.CANDIDATES_MAX_PER_ROW candidates.  Else (ids, cutoffs) as the engine takes them, and the engine holds the test
        matrix (with `ratings` where given), the `item_weights` and the candidate matrix the call needs.
        `evaluator_key`: a token the evaluator draws once from a process-wide counter (never id(): ids of freed objects are
        reused), under which its test and candidate matrices are uploaded once; the engine is compared by identity through a
        strong reference, so a rebuilt engine uploads again.  The item weights are uploaded again whenever their values change."""
        ready = self._device_ranking_args(user_id_array, cutoffs, max_cutoff, candidates_csr)
        if ready is None:
            return None
        ids, cutoffs = ready
        cand = candidates_csr is not None
        held = getattr(self, "_test_on_device", None)
        if (held is None or held.key != evaluator_key or held.engine is not self.engine
                or (ratings is not None and not held.has_ratings)):
            self.engine.set_test(urm_test_sorted, gains)
            if ratings is not None:
                self.engine.set_test_ratings(ratings)
            self._test_on_device = _TestOnDevice(evaluator_key, self.engine, ratings is not None)
        if item_weights is not None:
            held = getattr(self, "_weights_on_device", None)
            if (held is None or held[1] is not self.engine or not all(np.array_equal(a, b) for a, b in zip(held[0], item_weights))):
                self.engine.set_eval_item_weights(*item_weights)
                self._weights_on_device = (tuple(np.array(w, dtype=np.float64) for w in item_weights), self.engine)
        if cand:
            self._candidates_on_device(candidates_csr, key=evaluator_key)
        return ids, cutoffs

    def evaluate_on_device(self, evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, disc, ideal_cum,
                           remove_seen_flag=True, remove_CustomItems_flag=False):
        """Hold-out metric sums for EvaluatorHoldoutFast without leaving the device (ganmf_evaluate): [len(cutoffs), 9]
        float64 in the order of ganmf_amd._lib.EVAL_METRICS, or None when the device route does not apply (cut-off beyond
        the device selection, too many cut-offs).  The test matrix is uploaded once per evaluator (`evaluator_key`).
        `remove_CustomItems_flag` (here and on the sibling hooks): the items of set_items_to_ignore() are never ranked, as in
        recommend()."""
        ready = self._prepare_device_evaluation(evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, self._DEVICE_TOPK_MAX)
        if ready is None:
            return None
        with self._ignored_items(remove_CustomItems_flag):
            return self.engine.evaluate(ready[0], ready[1], disc, ideal_cum, transposed=(self.mode == 'item'),
                                        remove_seen=remove_seen_flag)

    def evaluate_full_on_device(self, evaluator_key, urm_test_sorted, gains, ratings, item_weights, user_id_array, cutoffs,
                                disc, ideal_cum, remove_seen_flag=True, counts=None, remove_CustomItems_flag=False):
        """The reference's full metric row for EvaluatorHoldoutFast(full_metrics=True) (ganmf_evaluate_full): returns the
        [len(cutoffs), 13] float64 sums of ganmf_amd._lib.EVAL_FULL_METRICS and adds the per-item counts of the lists into
        `counts` ([len(cutoffs), n_items] int64), or None when the device route does not apply (as evaluate_on_device).
        `ratings`: float32 per stored test entry; `item_weights`: the (novelty, popularity) pair of
        ganmf_amd.evaluation.popularity_weights, uploaded again whenever their values change."""
        ready = self._prepare_device_evaluation(evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, self._DEVICE_TOPK_MAX,
                                                ratings=ratings, item_weights=item_weights)
        if ready is None:
            return None
        with self._ignored_items(remove_CustomItems_flag):
            return self.engine.evaluate_full(ready[0], ready[1], disc, ideal_cum, transposed=(self.mode == 'item'),
                                             remove_seen=remove_seen_flag, counts=counts)[0]

    # ---- per-user candidate lists (Base/Evaluation/Evaluator.py:419-590, EvaluatorNegativeItemSample) ----------------
    @property
    def honours_items_to_compute(self):
        """whether `recommend(..., items_to_compute=...)` restricts the ranking: only under the MF contract (the reference's GANMF
        accepts the argument and ignores it, GANMF.py:285-292)"""
        return self.score_contract == "mf"

    def _candidates_on_device(self, candidates_csr, key=None):
        """uploads the candidate matrix unless the engine already holds the one of this `key` (an evaluator's device token)"""
        held = getattr(self, "_cand_on_device", None)
        if key is None or held is None or held[0] != key or held[1] is not self.engine:
            m = sps.csr_matrix(candidates_csr)
            if m.shape != (self.n_users, self.n_items):
                raise ValueError("candidates must be a %d x %d matrix, given %r" % (self.n_users, self.n_items, m.shape))
            self.engine.set_candidates(m)
            self._cand_on_device = (key, self.engine)

    def recommend_candidates(self, user_id_array, candidates_csr, cutoff, remove_seen_flag=True, candidates_key=None,
                             remove_CustomItems_flag=False):
        """Top-`cutoff` item ids of every user AMONG THAT USER'S OWN CANDIDATES, the stored entries of row `user` of
        `candidates_csr` (users x items, e.g. EvaluatorNegativeItemSample.URM_items_to_rank): an [n, cutoff] int32 array, -1 padded
        where a user has fewer unmasked candidates; ties go to the smaller item id.  Candidate scoring, seen-item mask and
        selection run in one HIP kernel (ganmf_recommend_candidates); no full-width score row is formed.  This is an explicit
        API, not the reference's `recommend`: it restricts to the candidates under either score contract (the cold-user mask
        stays the contract's).  `candidates_key`: a token that names this candidate matrix (an evaluator's device token); calls
        with the same token reuse the matrix the device already holds instead of uploading it again.  A cut-off above
        _lib.RECOMMEND_MAX_CUTOFF or a requested user with more than _lib.CANDIDATES_MAX_PER_ROW candidates is an error
        (ValueError / GanmfError)."""
        self._require_engine()
        ids = np.atleast_1d(np.asarray(user_id_array)).reshape(-1)
        if not 1 <= cutoff <= self.n_items:
            raise ValueError("recommend_candidates: cutoff %r outside [1, %d]" % (cutoff, self.n_items))
        self._candidates_on_device(candidates_csr, key=candidates_key)
        with self._ignored_items(remove_CustomItems_flag):
            items, _ = self.engine.recommend_candidates(ids, cutoff, transposed=(self.mode == 'item'), remove_seen=remove_seen_flag)
        return items

    def evaluate_candidates_on_device(self, evaluator_key, urm_test_sorted, gains, candidates_csr, user_id_array, cutoffs, disc,
                                      ideal_cum, remove_seen_flag=True, ratings=None, item_weights=None, counts=None,
                                      remove_CustomItems_flag=False):
        """Metric sums for EvaluatorNegativeItemSampleFast without leaving the device (ganmf_evaluate_candidates): every user
        ranked among the stored entries of its row of `candidates_csr`.  `ratings` None: [len(cutoffs), 9] float64 in the order
        of ganmf_amd._lib.EVAL_METRICS; `ratings` and `item_weights` given (full row): the [len(cutoffs), 13] sums of
        EVAL_FULL_METRICS, the lists' per-item counts added into `counts`.  The test and candidate matrices are uploaded once
        per evaluator (`evaluator_key`).
        Returns None -- the evaluator then takes another route -- under score_contract="ganmf" (the reference's GANMF ignores
        items_to_compute, so the reference's evaluator around it ranks the whole catalogue), for cut-offs the device selection
        does not take, and when a requested user has more than _lib.CANDIDATES_MAX_PER_ROW candidates."""
        full = ratings is not None
        ready = self._prepare_device_evaluation(evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, L.RECOMMEND_MAX_CUTOFF,
                                                ratings=ratings, item_weights=item_weights if full else None,
                                                candidates_csr=candidates_csr)
        if ready is None:
            return None
        with self._ignored_items(remove_CustomItems_flag):
            got = self.engine.evaluate_candidates(ready[0], ready[1], disc, ideal_cum, transposed=(self.mode == 'item'),
                                                  remove_seen=remove_seen_flag, counts=counts, full=full)
        return got[0] if full else got

    def evaluate_groups_on_device(self, evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs, disc, ideal_cum, group_of,
                                  n_groups, remove_seen_flag=True, candidates_csr=None, per_user=False, remove_CustomItems_flag=False):
        """Hold-out metrics per group of users without leaving the device (ganmf_evaluate_groups): (sums [n_groups, len(cutoffs), 9]
        float64 in the order of ganmf_amd._lib.EVAL_METRICS, sizes [n_groups], the [n, len(cutoffs), 9] per-user values or None).
        `group_of[i]` in [-1, n_groups) names the group of user_id_array[i] (-1: none).  `candidates_csr` None: the ranking of
        evaluate_on_device; given: every user among its own candidates, as evaluate_candidates_on_device.  The test (and candidate)
        matrix is uploaded once per evaluator (`evaluator_key`).  Returns None under the conditions of those two methods: cut-offs
        the device selection does not take, more than _lib.EVAL_MAX_CUTOFFS of them, and on the candidate route also
        score_contract != "mf" and a requested user with more than _lib.CANDIDATES_MAX_PER_ROW candidates; and for more than
        _lib.EVAL_MAX_GROUPS groups."""
        self._require_engine()
        cand = candidates_csr is not None
        if not 0 <= n_groups <= L.EVAL_MAX_GROUPS:
            return None
        ready = self._prepare_device_evaluation(evaluator_key, urm_test_sorted, gains, user_id_array, cutoffs,
                                                L.RECOMMEND_MAX_CUTOFF if cand else self._DEVICE_TOPK_MAX,
                                                candidates_csr=candidates_csr)
        if ready is None:
            return None
        with self._ignored_items(remove_CustomItems_flag):
            return self.engine.evaluate_groups(ready[0], ready[1], disc, ideal_cum, group_of, n_groups, transposed=(self.mode == 'item'),
                                               remove_seen=remove_seen_flag, candidates=cand, per_user=per_user)

    def evaluate_diversity_on_device(self, evaluator_key, matrix, user_id_array, cutoffs, remove_seen_flag=True, candidates_csr=None,
                                     remove_CustomItems_flag=False):
        """Sums over the users of the intra-list diversity of their ranked lists (DIVERSITY_SIMILARITY, metrics.py:405-452) without
        leaving the device (ganmf_evaluate_diversity): [len(cutoffs)] float64.  `matrix`: the [n_items, n_items] float32 item
        diversity matrix, uploaded once per `evaluator_key` and engine.  The ranking is evaluate_on_device's, or with
        `candidates_csr` evaluate_candidates_on_device's (every user among its own candidates); returns None where those return
        None.  A list with fewer than two items at a cut-off contributes 0 (the reference would divide by zero)."""
        cand = candidates_csr is not None
        ready = self._device_ranking_args(user_id_array, cutoffs, L.RECOMMEND_MAX_CUTOFF if cand else self._DEVICE_TOPK_MAX,
                                          candidates_csr)
        if ready is None:
            return None
        held = getattr(self, "_diversity_on_device", None)
        if held is None or held[0] != evaluator_key or held[1] is not self.engine:
            if np.shape(matrix) != (self.n_items, self.n_items):
                raise ValueError("the item diversity matrix must be %d x %d, given %r" % (self.n_items, self.n_items, np.shape(matrix)))
            self._diversity_on_device = None
            self.engine.set_item_diversity(matrix)
            self._diversity_on_device = (evaluator_key, self.engine)
        if cand:
            self._candidates_on_device(candidates_csr, key=evaluator_key)
        with self._ignored_items(remove_CustomItems_flag):
            return self.engine.evaluate_diversity(ready[0], ready[1], transposed=(self.mode == 'item'), remove_seen=remove_seen_flag,
                                                  candidates=cand)

    def activity_study(self, URM_test, bounds, cutoff=20, metric="MAP"):
        """ganmf_amd.studies.activity_study(self, ...): the reference's user-activity study (MFLearned.py:80-145) on the device"""
        from .studies import activity_study
        return activity_study(self, URM_test, bounds, cutoff=cutoff, metric=metric)

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None,
                  remove_top_pop_flag=False, remove_CustomItems_flag=False, return_scores=False):
        device_ok = (not return_scores and cutoff is not None and 1 <= cutoff <= self._DEVICE_TOPK_MAX
                     and cutoff <= self.n_items)
        if not device_ok:   # full score matrix needed on the host: the reference's own route
            saved = self.URM_train
            self.URM_train = self._URM_eval
            try:
                return super(DeviceScoringMixin, self).recommend(user_id_array, cutoff=cutoff, remove_seen_flag=remove_seen_flag,
                                                    items_to_compute=items_to_compute,
                                                    remove_top_pop_flag=remove_top_pop_flag,
                                                    remove_CustomItems_flag=remove_CustomItems_flag,
                                                    return_scores=return_scores)
            finally:
                self.URM_train = saved
        single = np.isscalar(user_id_array)
        items = self.recommend_topk(user_id_array, cutoff, remove_seen_flag, items_to_compute=items_to_compute,
                                    remove_CustomItems_flag=remove_CustomItems_flag, remove_top_pop_flag=remove_top_pop_flag)
        lists = [row[row >= 0].tolist() for row in items]
        return lists[0] if single else lists
