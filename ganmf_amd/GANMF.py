"""GANMF recommender — host mirror of the reference class (GANRec/GANMF.py:23-342).

Same constructor, fit() keyword arguments, return-value quirk, scoring and early-stopping hooks
as the reference, so it can stand in for `GANRec.GANMF.GANMF` under RecSysExp.py /
RunBestParameters.py.  Every number is produced by libganmf_hip.so (HIP kernels on gfx950)
through the C ABI in include/ganmf_hip.h; this file holds only the epoch loop and bookkeeping.
"""
import collections
import contextlib
import os
import pickle
import time
from datetime import datetime

import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .early_stopping import EarlyStoppingScheduler
from .engine import Engine
from .evaluation import _pad_lists

try:  # progress bar is cosmetic (GANMF.py:170,234)
    import tqdm
except Exception:  # pragma: no cover
    tqdm = None


def glorot_uniform(rng, shape):
    """tf.glorot_uniform_initializer for [a, b] variables (GANMF.py:57): U(-L, L), L = sqrt(6/(a+b)).
    TF's seeded Philox stream cannot be reproduced without TF; the build's documented default is
    numpy RandomState(seed) drawing, in order, encoding/kernel, decoding/kernel, user_embeddings,
    item_embeddings (biases are zero, tf.layers.dense default)."""
    limit = np.sqrt(6.0 / (shape[0] + shape[1]))
    return rng.uniform(-limit, limit, size=shape).astype(np.float32)


class _TensorRef(object):
    """Stands where the reference keeps tf.Variable objects in model.params (GANMF.py:119-122)."""

    def __init__(self, tid, name):
        self.tid, self.name = tid, name


# the test matrix an engine holds for device evaluation: the evaluator's token, that engine, whether the ratings went up with it
_TestOnDevice = collections.namedtuple("_TestOnDevice", "key engine has_ratings")


class _SessionShim(object):
    """model.sess.run(var) -> ndarray, the only use callers make of the session (Utils_.py:305-308)."""

    def __init__(self, model):
        self._model = model

    def run(self, fetch):
        if isinstance(fetch, (list, tuple)):
            return [self.run(f) for f in fetch]
        if not isinstance(fetch, _TensorRef):
            raise TypeError("only parameter handles can be fetched")
        return self._model._get(fetch.tid)


class GANMF(BaseRecommender):
    RECOMMENDER_NAME = 'GANMF'

    # (tensor id, reference variable name, attribute for shape)
    _D_TENSORS = ((0, 'autoencoder/encoding/kernel'), (1, 'autoencoder/encoding/bias'),
                  (2, 'autoencoder/decoding/kernel'), (3, 'autoencoder/decoding/bias'))
    _G_TENSORS = ((L.T_USER_EMB, 'generator/user_embeddings'), (L.T_ITEM_EMB, 'generator/item_embeddings'))

    SCORE_CONTRACTS = ("ganmf", "mf")

    def __init__(self, URM_train, mode='user', verbose=False, seed=1234, is_experiment=False, device=0, devices=None,
                 dist_backend=None, world_size=None, score_contract=None):
        """`score_contract` (beyond the reference's signature; also GANMF_SCORE_CONTRACT in the environment) selects what
        `_compute_item_score` / `recommend` / the device evaluator return for the two corners the reference's classes differ in:
          "ganmf" (default) = GANRec/GANMF.py:285-292 exactly: the class derives from BaseRecommender, every user -- with or
                    without a training interaction -- gets the finite scores U[ids] . V^T, and `items_to_compute` is accepted
                    and ignored;
          "mf"    = Base/BaseMatrixFactorizationRecommender.py:113-119,128-143, the contract the north star names: only
                    `items_to_compute` keep their scores (the others -inf) and users without a training interaction score
                    -inf everywhere (empty recommendation lists).
        `devices` (beyond the reference's signature; also GANMF_DEVICES="0,1,2,3" in the environment, so that the
        reference's drivers need no change): fit() shards the generator's users row-wise over these GPUs, one rank process
        per GPU over RCCL (ganmf_amd/dist.py ShardedEngine; north star: "users shard row-wise across the 8 GPUs of one
        node").  dist_backend="local" + world_size=N (GANMF_DIST_BACKEND / GANMF_WORLD_SIZE) puts N ranks on ONE GPU over the
        library's loopback communicator (tests).  Default: one GPU, `device`."""
        if mode not in ['user', 'item']:
            raise ValueError('Accepted training modes are `user` and `item`. Given was {}.', mode)
        self.mode = mode
        # the reference does not call super().__init__ (GANMF.py:26-51); keep its attributes
        URM_train = sps.csr_matrix(URM_train, dtype=np.float32)
        self._URM_eval = URM_train                       # user x item, what evaluators see
        self._URM_fit = URM_train.T.tocsr() if mode == 'item' else URM_train   # training orientation
        self.URM_train = self._URM_fit                   # GANMF.py:31-35
        self.num_users, self.num_items = self.URM_train.shape
        self.n_users, self.n_items = URM_train.shape
        self.config = None
        self.seed = seed
        self.verbose = verbose
        self.device = device
        if devices is None and os.environ.get("GANMF_DEVICES"):
            devices = [int(d) for d in os.environ["GANMF_DEVICES"].split(",") if d.strip() != ""]
        self.devices = list(devices) if devices is not None else None
        self.dist_backend = dist_backend or os.environ.get("GANMF_DIST_BACKEND") or "process"
        self.world_size = world_size if world_size is not None else (int(os.environ["GANMF_WORLD_SIZE"]) if os.environ.get("GANMF_WORLD_SIZE") else None)
        self.score_contract = score_contract or os.environ.get("GANMF_SCORE_CONTRACT") or "ganmf"
        if self.score_contract not in self.SCORE_CONTRACTS:
            raise ValueError("score_contract must be one of %r, given %r" % (self.SCORE_CONTRACTS, self.score_contract))
        self.logsdir = os.path.join('plots', self.RECOMMENDER_NAME, datetime.now().strftime("%Y%m%d-%H%M%S"))
        self.is_experiment = is_experiment
        if not self.is_experiment:
            os.makedirs(self.logsdir, exist_ok=True)
        self.items_to_ignore_flag = False
        self.items_to_ignore_ID = np.array([], dtype=int)
        self.filterTopPop = False
        self.filterTopPop_ItemsID = np.array([], dtype=int)
        self.mfma = None                # None | "f32" | "bf16" | "f16": arithmetic of the GEMM K loops (engine.Engine)
        self.initial_weights = None     # optional dict {We,be,Wd,bd,U,V}: explicit init (parity tests)
        self.schedule_rng = None        # optional numpy RandomState for the per-epoch shuffle instead of numpy's GLOBAL stream (the
                                        # reference's, GANMF.py:175): RandomState(s) draws what np.random.seed(s) would, and lets
                                        # several fits run in threads of one process (tune.py: engines_per_worker)
        self.engine = None
        self.params = None
        self.sess = None
        self._stop_training = False
        self.train_d_loss, self.train_g_loss = [], []

    # ---- engine plumbing -----------------------------------------------------------------------
    _NAME2ID = {"We": 0, "be": 1, "Wd": 2, "bd": 3, "U": L.T_USER_EMB, "V": L.T_ITEM_EMB}

    def _get(self, tid):
        a = self.engine.get_tensor(tid)
        return a[0] if tid in (1, 3) else a

    def _build(self, num_factors, emb_dim, batch_size, **hp):
        self.num_factors, self.emb_dim = num_factors, emb_dim
        if self.engine is not None:
            self.engine.close()
        self.engine = self._make_engine(num_factors, emb_dim, batch_size, mfma=self.mfma, **hp)
        self.engine.set_urm(self._URM_fit)
        self.engine.set_seen(self._URM_eval)            # for device-side recommend()
        self._reset_score_filter()
        self.params = {'D': [_TensorRef(t, n) for t, n in self._D_TENSORS],
                       'G': [_TensorRef(t, n) for t, n in self._G_TENSORS]}
        self.sess = _SessionShim(self)

    def _reset_score_filter(self):
        """no item filter; the cold-user mask only under the MF contract (the reference's GANMF scores every user)"""
        self.engine.set_score_filter(None, mask_cold=(self.score_contract == "mf"))

    def _sharded(self):
        if self.dist_backend == "local":
            return (self.world_size or 1) > 1
        return self.devices is not None and len(self.devices) > 1

    def _make_engine(self, num_factors, width, batch_size, **kw):
        """One Engine on `device`, or the row-sharded group (same methods) when several devices / ranks were asked for."""
        if not self._sharded():
            # a single entry in `devices` / GANMF_DEVICES names THE device (it used to be ignored in favour of `device`)
            dev = self.devices[0] if (self.devices is not None and len(self.devices) == 1 and self.dist_backend != "local") else self.device
            return Engine(self.num_users, self.num_items, num_factors, width, batch_size, device=dev, **kw)
        from .dist import ShardedEngine
        if self.dist_backend == "local":
            return ShardedEngine(self.num_users, self.num_items, num_factors, width, batch_size, world_size=self.world_size,
                                 devices=[self.devices[0] if self.devices else self.device], backend="local", **kw)
        return ShardedEngine(self.num_users, self.num_items, num_factors, width, batch_size, devices=self.devices,
                             backend="process", **kw)

    def _init_weights(self):
        if self.initial_weights is not None:
            w = self.initial_weights
        else:
            rng = np.random.RandomState(self.seed)
            w = {"We": glorot_uniform(rng, (self.num_items, self.emb_dim)),
                 "be": np.zeros(self.emb_dim, np.float32),
                 "Wd": glorot_uniform(rng, (self.emb_dim, self.num_items)),
                 "bd": np.zeros(self.num_items, np.float32),
                 "U": glorot_uniform(rng, (self.num_users, self.num_factors)),
                 "V": glorot_uniform(rng, (self.num_items, self.num_factors))}
        for name, tid in self._NAME2ID.items():
            self.engine.set_tensor(tid, w[name])

    # ---- fit (GANMF.py:88-244) -------------------------------------------------------------------
    def fit(self, num_factors=10, emb_dim=32, epochs=300, batch_size=32, d_lr=1e-4, g_lr=1e-4, d_steps=1, g_steps=1,
            d_reg=0, g_reg=0, m=1, recon_coefficient=1e-2, allow_worse=None, freq=None, after=0, metrics=['MAP'],
            sample_every=None, validation_evaluator=None, validation_set=None):
        self.config = dict(locals())
        del self.config['self']

        self._build(num_factors, emb_dim, batch_size, d_lr=d_lr, g_lr=g_lr, d_reg=d_reg, g_reg=g_reg, m=m,
                    recon_coefficient=recon_coefficient)
        self._init_weights()

        return self._epoch_loop(epochs, d_steps, g_steps, allow_worse, freq, after, metrics, sample_every,
                                validation_evaluator, validation_set)

    def _epoch_loop(self, epochs, d_steps, g_steps, allow_worse, freq, after, metrics, sample_every,
                    validation_evaluator, validation_set):
        """Epochs 1..`epochs` shared by GANMF and DisGANMF (schedule of GANMF.py:151-244, DisGANMF.py:152-244).

        Per epoch: ONE in-place shuffle of the row ids on numpy's global stream (cumulative across epochs, which is
        what makes a seeded run reproduce the reference's minibatch schedule, GANMF.py:175), ONE library call that
        runs `d_steps` passes of discriminator updates and then `g_steps` passes of generator updates over the same
        slices of that permutation (:176-203), then the optional progress evaluation and the early-stopping hook.
        Returns the epoch early stopping fired at, or `epochs + 1` when it never did (the reference's counter is
        incremented once more before its loop ends, :244 -- callers subtract `allow_worse * freq` from it)."""
        self._stop_training = False
        watcher = None
        if validation_evaluator is not None:
            watcher = EarlyStoppingScheduler(self, evaluator=validation_evaluator, allow_worse=allow_worse, freq=freq,
                                             metrics=metrics, after=after)
        row_ids = np.arange(self.num_users)
        self.train_d_loss, self.train_g_loss = [], []
        progress = tqdm.tqdm(total=epochs, initial=1) if (tqdm is not None and self.verbose) else None
        if self.verbose:
            print('Starting training...')
        fit_t0 = window_t0 = time.time()
        stopped_at = None
        for epoch in range(1, epochs + 1):
            (self.schedule_rng if self.schedule_rng is not None else np.random).shuffle(row_ids)
            d_losses, g_losses = self.engine.train_epoch(row_ids, d_steps, g_steps)
            self.train_d_loss.append(np.mean(d_losses) if len(d_losses) else np.nan)
            self.train_g_loss.append(np.mean(g_losses) if len(g_losses) else np.nan)

            if validation_set is not None and sample_every is not None and epoch % sample_every == 0:
                elapsed = time.time() - window_t0
                print('Epoch : {:d}. Total: {:.2f} secs, {:.2f} secs/epoch.'.format(epoch, elapsed, elapsed / sample_every))
                print(self._evaluate_in_eval_orientation(lambda: validation_evaluator.evaluateRecommender(self)[1]))
                window_t0 = time.time()
            if watcher is not None:
                self._evaluate_in_eval_orientation(lambda: watcher(epoch))
            if progress is not None:
                progress.update()
            if self._stop_training:
                print('Training stopped, epoch:', epoch)
                stopped_at = epoch
                break
        if progress is not None:
            progress.close()
        if self.verbose:
            print('Training took {:.2f} seconds'.format(time.time() - fit_t0))
        self.URM_train = self._URM_eval      # user x item again once fit() returns (GANMF.py:241-242)
        return epochs + 1 if stopped_at is None else stopped_at

    def _evaluate_in_eval_orientation(self, call):
        """Runs `call()` with self.URM_train in user x item orientation (what evaluators and remove-seen expect)
        and switches back to the training orientation afterwards."""
        self._flip_for_evaluation(True)
        try:
            return call()
        finally:
            self._flip_for_evaluation(False)

    def _flip_for_evaluation(self, to_eval):
        """The reference flips self.URM_train with .T.tocsr() around every evaluation in item mode
        (GANMF.py:215-228); both orientations are kept instead of re-transposing."""
        self.URM_train = self._URM_eval if to_eval else self._URM_fit

    # ---- hooks used by EarlyStoppingScheduler (GANMF.py:246-255) --------------------------------
    def stop_fit(self):
        self._stop_training = True

    def save_current_model(self):
        self.engine.snapshot_best()

    def load_model(self):
        self.engine.restore_best()

    def load_weights(self, best_params, weights):
        """GANMF.py:257-283: `weights` is the Utils_.saveWeights dict {'D': [...], 'G': [...]}."""
        self._build(best_params['num_factors'], best_params['emb_dim'], batch_size=32)
        for ref, w in zip(self.params['D'] + self.params['G'], list(weights['D']) + list(weights['G'])):
            self.engine.set_tensor(ref.tid, np.asarray(w, dtype=np.float32))

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

        class _Ctx(object):
            def __enter__(self_inner):
                eng.set_score_filter(items_to_compute, mask_cold=True)

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
                return super(GANMF, self).recommend(user_id_array, cutoff=cutoff, remove_seen_flag=remove_seen_flag,
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

    def _require_engine(self):
        if self.engine is None:
            raise RuntimeError("GANMF: model has no device state; call fit() or loadModel() first")

    def user_factors(self):
        self._require_engine()
        return self._get(L.T_USER_EMB)

    def item_factors(self):
        self._require_engine()
        return self._get(L.T_ITEM_EMB)

    # MF contract named by the north star (BaseMatrixFactorizationRecommender.py:94-143):
    # USER_factors[ids] @ ITEM_factors.T == _compute_item_score(ids), evaluation orientation
    @property
    def USER_factors(self):
        return self.item_factors() if self.mode == 'item' else self.user_factors()

    @property
    def ITEM_factors(self):
        return self.user_factors() if self.mode == 'item' else self.item_factors()

    # ---- the discriminator's view of a profile (ganmf_discriminate) --------------------------------
    def _discriminator_rows(self, row_ids):
        """generator rows in training orientation (item mode: catalogue items); None = all of them"""
        if row_ids is None:
            return np.arange(self.num_users, dtype=np.int32)
        return np.atleast_1d(np.asarray(row_ids)).reshape(-1).astype(np.int32)

    def autoencoder_codes(self, row_ids=None, generated=False):
        """GANMF.py:304-307: the encoding E = x . We + be of every training row -- [num_users, emb_dim] float32, training
        orientation -- or of the rows `row_ids`; with generated=True of their generated profiles U[row_ids] . V^T instead of
        the stored ones.  Formed on the device (ganmf_discriminate: a CSR row-sum over the stored entries; the matrix is
        never densified).  This method used to fetch the encoder and run a scipy product on the host: the route changed,
        the signature of the no-argument call, its shape and its dtype did not."""
        self._require_engine()
        return self.engine.discriminate(self._discriminator_rows(row_ids), generated=generated, features=True, value=False)[0]

    def discriminator_energy(self, row_ids=None, generated=False):
        """The EBGAN energy the discriminator assigns to each row, D(x) = mean_j (dec(enc(x)) - x)_j^2 -- the
        tf.losses.mean_squared_error of GANMF.py:68 taken per row instead of per batch -- for the stored profiles of
        `row_ids` (None: every training row) or, with generated=True, for their generated profiles.  float64 [n], formed on
        the device; the reconstruction never leaves it."""
        self._require_engine()
        return self.engine.discriminate(self._discriminator_rows(row_ids), generated=generated, features=False, value=True)[1]

    def discriminator_study(self, row_ids=None):
        """ganmf_amd.studies.discriminator_study(self, ...): real against generated rows as the discriminator sees them"""
        from .studies import discriminator_study
        return discriminator_study(self, row_ids=row_ids)

    # ---- persistence (GANMF.py:309-342) -----------------------------------------------------------
    # Same files as the reference: build_params.pkl + the tf.train.Saver bundle <name>.index /
    # <name>.data-00000-of-00001 holding params['D'] + params['G'] (ganmf_amd/tf_bundle.py), so models
    # saved by either side load on the other (AblationStudy.py:85-88, MFLearned.py:95).
    def _model_file(self, folder_path, file_name):
        return os.path.join(folder_path, self.RECOMMENDER_NAME + '_' + self.mode if file_name is None else file_name)

    def saveModel(self, folder_path, file_name=None):
        from .tf_bundle import write_bundle
        self._require_engine()
        os.makedirs(folder_path, exist_ok=True)
        build_params = {'num_factors': self.num_factors, 'emb_dim': self.emb_dim}
        with open(os.path.join(folder_path, 'build_params.pkl'), 'wb') as f:
            pickle.dump(build_params, f, pickle.HIGHEST_PROTOCOL)
        write_bundle(self._model_file(folder_path, file_name),
                     {ref.name: self.sess.run(ref) for ref in self.params['D'] + self.params['G']})

    def loadModel(self, folder_path, file_name=None):
        from .tf_bundle import read_bundle
        filepath = os.path.join(folder_path, 'build_params.pkl')
        if self.verbose:
            print(self.RECOMMENDER_NAME + ': Loading model from file ' + filepath)
        with open(filepath, 'rb') as f:
            build_params = pickle.load(f)
        data = read_bundle(self._model_file(folder_path, file_name))
        self._build(build_params['num_factors'], build_params['emb_dim'], batch_size=32)
        for ref in self.params['D'] + self.params['G']:
            if ref.name not in data:
                raise KeyError("%s: checkpoint has no tensor %r" % (self.RECOMMENDER_NAME, ref.name))
            self.engine.set_tensor(ref.tid, data[ref.name])
        if self.verbose:
            print(self.RECOMMENDER_NAME + ': Loading complete')
