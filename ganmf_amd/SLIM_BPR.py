"""SLIM_BPR_Cython -- SLIM trained with BPR, host mirror of the reference class (SLIM_BPR/Cython/SLIM_BPR_Cython.py:50-199; the SLIMBPR
row of the comparison table in RecSysExp.py:71-97).

Same constructor, fit() keyword arguments, early-stopping keyword arguments, W_sparse layout and saved-model layout as the reference, so
it can stand in for `SLIM_BPR.Cython.SLIM_BPR_Cython.SLIM_BPR_Cython`.  The training -- the reference's Cython epoch, one sample after
another in float64 -- runs in libganmf_hip.so (ganmf_slim_bpr_*: HIP kernels on gfx950, on a GANMF_MODEL_ITEMSIM handle): S and the
optimiser state stay on the device, where get_S, the column top-K, scoring -- URM_train[users] . W_sparse -- recommendation and
evaluation run as well.  This file holds what the reference decides on the host: the positive_threshold_BPR filter, the argument
checks, the epoch loop with its early stopping (EarlyStoppingMixin) and the quirks below.

Kept from the reference, as it behaves:
  * W_sparse[a, b] = S[a, b]: the scores sum S[s, j] over the profile although the training sums S[j, s] (it matters when symmetric
    is False);
  * the model left by fit() is the one of the LAST epoch: S_best is maintained and never read;
  * batch_size is stored and not used: an epoch is n_users + 1 samples applied one after another.
Departures:
  * train_with_sparse_weights = True raises ValueError (the tree-CSR mode prunes S during training and is not built); None means dense;
  * recompile_cython is accepted and ignored;
  * random_seed: the reference never forwards it to its epoch object, whose C rand() stream is therefore not replayable.  Here an
    integer seeds the device sampler as given, and None takes the seed from numpy's global stream, so np.random.seed() governs a run
    as it does for PureSVDRecommender."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .incremental_training import EarlyStoppingMixin
from .similarity_model import SimilarityModelMixin


def row_topk_csr(S, k):
    """get_S on the host, for S_incremental / S_best: the diagonal zeroed, the k largest of every row (ties to the smaller id), the
    non-zero ones kept; float64 CSR, columns ascending"""
    S = np.array(S, dtype=np.float64)
    n = S.shape[0]
    np.fill_diagonal(S, 0.0)
    k = min(int(k), n)
    if k < n:
        # the k-th largest value of every row; everything above it is kept, and of the entries equal to it the first ones (smaller ids)
        kth = -np.partition(-S, k - 1, axis=1)[:, k - 1:k]
        above, equal = S > kth, S == kth
        room = k - above.sum(axis=1, keepdims=True)
        S = np.where(above | (equal & (np.cumsum(equal, axis=1) <= room)), S, 0.0)
    out = sps.csr_matrix(S)
    out.eliminate_zeros()
    out.sort_indices()
    return out


class SLIM_BPR_Cython(EarlyStoppingMixin, SimilarityModelMixin, DeviceScoringMixin, BaseRecommender):
    RECOMMENDER_NAME = "SLIM_BPR_Recommender"

    MAX_TOPK = L.ITEMKNN_MAX_TOPK

    # what the device-scoring surface reads: as ItemKNNCFRecommender
    mode = "user"
    score_contract = "mf"
    mask_cold_users = False

    def __init__(self, URM_train, free_mem_threshold=0.5, recompile_cython=False, device=0, verbose=False):
        super(SLIM_BPR_Cython, self).__init__(URM_train)
        assert free_mem_threshold >= 0.0 and free_mem_threshold <= 1.0, \
            "SLIM_BPR_Recommender: free_mem_threshold must be between 0.0 and 1.0, provided was '{}'".format(free_mem_threshold)
        self._URM_eval = self.URM_train
        self.free_mem_threshold = free_mem_threshold      # (read by the reference's choice of the tree-CSR mode only)
        self.device = device
        self.verbose = verbose
        self.engine = None
        self._S_cache = None
        self._topk = None
        self.epochs_best = 0
        self.best_validation_metric = None
        self.train_route = L.SLIM_AUTO      # L.SLIM_SEQUENTIAL / L.SLIM_LEVELLED: the route of every epoch (the same bytes either way)

    def fit(self, epochs=300, positive_threshold_BPR=None, train_with_sparse_weights=None, symmetric=True, verbose=False,
            random_seed=None, batch_size=1000, lambda_i=0.0, lambda_j=0.0, learning_rate=1e-4, topK=200, sgd_mode='adagrad',
            gamma=0.995, beta_1=0.9, beta_2=0.999, **earlystopping_kwargs):
        if train_with_sparse_weights:
            raise ValueError("{}: train_with_sparse_weights=True (the tree-CSR mode, which prunes S during training) is not "
                             "implemented; pass None or False for the dense modes".format(self.RECOMMENDER_NAME))
        self.symmetric = symmetric
        self.train_with_sparse_weights = False
        self.positive_threshold_BPR = positive_threshold_BPR
        self.sgd_mode = sgd_mode
        self.epochs = epochs

        # Select only positive interactions (SLIM_BPR_Cython.py:118-130)
        URM_train_positive = self.URM_train.copy()
        if self.positive_threshold_BPR is not None:
            URM_train_positive.data = URM_train_positive.data >= self.positive_threshold_BPR
            URM_train_positive.eliminate_zeros()
            assert URM_train_positive.nnz > 0, "SLIM_BPR_Cython: URM_train_positive is empty, positive threshold is too high"
        if sgd_mode not in L.SLIM_SGD_MODES:
            raise ValueError("SGD_mode not valid. Acceptable values are: 'sgd', 'adagrad', 'rmsprop', 'adam'. Provided value was '{}'".format(
                sgd_mode))
        if topK is not False and topK < 1:
            raise ValueError("TopK not valid. Acceptable values are either False or a positive integer value. Provided value was '{}'".format(
                topK))
        topk = self.n_items if topK is False else min(int(topK), self.n_items)      # False: every non-zero is kept
        if topk > self.MAX_TOPK:
            raise ValueError("{}: topK must be at most {} (the device selection runs topK rounds per item), provided was {}".format(
                self.RECOMMENDER_NAME, self.MAX_TOPK, topK))
        self.topK = topK
        self._topk = topk
        self.batch_size = batch_size
        self.lambda_i = lambda_i
        self.lambda_j = lambda_j
        self.learning_rate = learning_rate
        self.random_seed = random_seed
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if random_seed is None else int(random_seed)

        profiles = sps.csr_matrix((np.ones(URM_train_positive.nnz, dtype=np.float32), URM_train_positive.indices, URM_train_positive.indptr),
                                  shape=URM_train_positive.shape, copy=True)
        profiles.sum_duplicates()
        profiles.sort_indices()
        self._build()      # the engine with URM_train (what the scores are formed from) and the seen mask
        self.engine.slim_bpr_init(symmetric=bool(symmetric), sgd_mode=sgd_mode, learning_rate=learning_rate, lambda_i=lambda_i,
                                  lambda_j=lambda_j, gamma=gamma, beta_1=beta_1, beta_2=beta_2, seed=seed, profiles=profiles)
        self._S_cache = sps.csr_matrix((self.n_items, self.n_items), dtype=np.float64)      # get_S of the zero matrix
        self.S_best = self.S_incremental.copy()
        self._train_with_early_stopping(epochs, **earlystopping_kwargs)
        self.get_S_incremental_and_set_W()

    @property
    def S_incremental(self):
        """the reference's get_S() of the current device state: float64 CSR, the top-K of every row of S (read back and selected on
        the host when asked for; the device keeps its own for W_sparse)"""
        self._require_engine()
        if self._S_cache is None:
            self._S_cache = row_topk_csr(self.engine.slim_bpr_state()["S"], self._topk)
        return self._S_cache

    def _prepare_model_for_validation(self):
        self.get_S_incremental_and_set_W()

    def _update_best_model(self):
        self.S_best = self.S_incremental.copy()

    def _run_epoch(self, num_epoch):
        self.engine.slim_bpr_epochs(1, mode=self.train_route)
        self._S_cache = None

    def get_S_incremental_and_set_W(self):
        """W_sparse from the current S, on the device: get_S, then the top-K of every column (SLIM_BPR_Cython.py:188-197)"""
        self._require_engine()
        self.engine.slim_bpr_finish(self._topk)
