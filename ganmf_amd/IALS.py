"""IALSRecommender -- implicit-feedback ALS (WRMF), host mirror of the reference class
(MatrixFactorization/IALSRecommender.py:15-210; "ALS" / "WRMF" in the learned-MF studies of MFLearned.py).

Same constructor, fit() keyword arguments, early-stopping attributes and saved-model layout as the reference, so it can stand in for
`MatrixFactorization.IALSRecommender.IALSRecommender` under RecSysExp.py / RunBestParameters.py.  Every factor is computed by
libganmf_hip.so: one epoch is two calls of ganmf_als_half_sweep (a Gram product and one Cholesky solve per warm row, HIP kernels on
gfx950) on a GANMF_MODEL_MF handle; scoring, recommendation and evaluation are the device routes of DeviceScoringMixin under the MF
contract (Base/BaseMatrixFactorizationRecommender.py:94-143).  This file holds the confidence scaling, the initial factors and the epoch
loop, whose early stopping is EarlyStoppingMixin's (incremental_training.py); the engine plumbing, the factor properties and persistence are
FactorModelMixin's (factor_model.py)."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .incremental_training import EarlyStoppingMixin
from .factor_model import FactorModelMixin


class IALSRecommender(EarlyStoppingMixin, FactorModelMixin, DeviceScoringMixin, BaseRecommender):
    RECOMMENDER_NAME = "IALSRecommender"

    AVAILABLE_CONFIDENCE_SCALING = ["linear", "log"]
    MAX_FACTORS = L.ALS_MAX_FACTORS
    MAX_FACTORS_REASON = "a row's system has to fit the LDS of a compute unit"

    # what the device-scoring surface reads: users are rows, and the MF contract always holds (IALSRecommender derives from
    # BaseMatrixFactorizationRecommender in the reference)
    mode = "user"
    score_contract = "mf"

    def __init__(self, URM_train, device=0, verbose=False):
        super(IALSRecommender, self).__init__(URM_train)
        self._URM_eval = self.URM_train
        self.device = device
        self.verbose = verbose
        self.use_bias = False
        self.engine = None
        self.num_factors = None
        self.epochs_best = 0
        self.best_validation_metric = None

    # ---- fit (IALSRecommender.py:40-126) -----------------------------------------------------------
    def _confidence(self, confidence_scaling, alpha, epsilon):
        """C in float32 on the host: 1 + alpha r, or 1 + alpha log(1 + r / epsilon), at the stored entries of URM_train"""
        C = sps.csr_matrix(self.URM_train, dtype=np.float32, copy=True)
        if confidence_scaling == "linear":
            C.data = (1.0 + alpha * C.data).astype(np.float32)
        else:
            C.data = (1.0 + alpha * np.log(1.0 + C.data / epsilon)).astype(np.float32)
        return C

    def fit(self, epochs=300, num_factors=20, confidence_scaling="linear", alpha=1.0, epsilon=1.0, reg=1e-3, init_mean=0.0,
            init_std=0.1, **earlystopping_kwargs):
        """The reference's fit().  init_mean / init_std are accepted and, as in the reference, not used: ITEM factors start as
        num_factors**-0.5 * random_sample on numpy's global stream, USER factors as zeros (the reference leaves them
        uninitialised; users without an interaction are never solved for and stay zero here)."""
        if confidence_scaling not in self.AVAILABLE_CONFIDENCE_SCALING:
            raise ValueError("Value for 'confidence_scaling' not recognized. Acceptable values are {}, provided was '{}'".format(
                self.AVAILABLE_CONFIDENCE_SCALING, confidence_scaling))
        self._build(num_factors)
        self.alpha, self.epsilon, self.reg = alpha, epsilon, reg
        C = self._confidence(confidence_scaling, alpha, epsilon)
        C_csc = C.tocsc()
        self.engine.set_confidence(0, C)
        self.engine.set_confidence(1, sps.csr_matrix((C_csc.data, C_csc.indices, C_csc.indptr), shape=(self.n_items, self.n_users)))
        self.engine.set_tensor(L.T_USER_EMB, np.zeros((self.n_users, self.num_factors), dtype=np.float32))
        self.engine.set_tensor(L.T_ITEM_EMB, self.num_factors ** -0.5 * np.random.random_sample((self.n_items, self.num_factors)))
        self._update_best_model()
        self._train_with_early_stopping(epochs, **earlystopping_kwargs)
        self.engine.restore_best()      # USER_factors = USER_factors_best, ITEM_factors = ITEM_factors_best

    def _run_epoch(self, num_epoch):
        self.engine.als_half_sweep(0, self.reg)      # users from items
        self.engine.als_half_sweep(1, self.reg)      # items from the new users

    def _update_best_model(self):
        """the best factors stay on the device, in the handle's `best` slots"""
        self.engine.snapshot_best()
