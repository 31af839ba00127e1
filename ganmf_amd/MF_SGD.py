"""MatrixFactorization_BPR_Cython, MatrixFactorization_FunkSVD_Cython and MatrixFactorization_AsySVD_Cython -- the SGD matrix
factorisations, host mirror of the reference classes (MatrixFactorization/Cython/MatrixFactorization_Cython.py:19-330).

Same constructors, fit() keyword arguments, early-stopping keyword arguments, members and saved-model layout as the reference, so they
can stand in for `MatrixFactorization.Cython.MatrixFactorization_Cython.*`.  The training -- the reference's Cython epoch, mini-batches
in float64 -- runs in libganmf_hip.so (ganmf_mf_sgd_*: HIP kernels on gfx950, on a GANMF_MODEL_MF handle): the factors, the biases and
the optimiser state stay on the device in float64; ganmf_mf_sgd_publish rounds them into the handle's float32 factor tensors (the
biases as two more columns), from which scoring, recommendation, evaluation and the best slot run as for IALSRecommender.  This file
holds what the reference decides on the host: the positive_threshold_BPR filter, the float32 rounding of the rates, the initial
factors, the argument checks, the epoch loop with its early stopping (EarlyStoppingMixin) and the quirks below.

Kept from the reference, as it behaves:
  * FunkSVD's item gradient uses positive_reg, which FunkSVD's fit() never passes: items are not regularised and item_reg has no effect;
  * negative_interactions_quota, once non-zero, is the probability of a POSITIVE sample (sampleMSE_Cython draws a positive when
    rand() <= quota RAND_MAX); a sampled negative has rating 0;
  * the model left by fit() is the one of the best validation, not of the last epoch (unlike SLIM_BPR_Cython);
  * learning_rate and the regularisation weights are rounded to float32 (C float members); gamma, beta_1 and beta_2 are fixed at
    0.995, 0.9 and 0.999 (fit() never forwards them);
  * MatrixFactorization_BPR_Cython forces use_bias = False and negative_interactions_quota = 0.
Departures:
  * MatrixFactorization_AsySVD_Cython.fit() raises NotImplementedError: the reference's batch update reads the profile bounds and the
    accumulated user vector of the LAST sample drawn in the batch's first phase, not of the sample being applied
    (MatrixFactorization_Cython_Epoch.pyx:541-576); restating that is not worth a kernel;
  * recompile_cython is accepted and ignored;
  * random_seed seeds numpy (the initial factors are the reference's own bytes) and the device sampler, whose stream is not C rand()'s;
    None takes the sampler's seed from numpy's global stream."""
import io
import json
import zipfile

import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .factor_model import FactorModelMixin
from .incremental_training import EarlyStoppingMixin

SGD_MODE_VALUES = ["sgd", "adam", "adagrad", "rmsprop"]
ALGORITHM_NAME_VALUES = ["FUNK_SVD", "ASY_SVD", "MF_BPR"]
_MEMBERS = ("USER_factors", "ITEM_factors", "USER_bias", "ITEM_bias", "GLOBAL_bias")


def float32_value(x):
    """x as a C float member holds it, widened back to a double"""
    return float(np.float32(x))


class _MatrixFactorization_Cython(EarlyStoppingMixin, FactorModelMixin, DeviceScoringMixin, BaseRecommender):
    RECOMMENDER_NAME = "MatrixFactorization_Cython_Recommender"

    MAX_FACTORS = L.MF_SGD_MAX_FACTORS
    MAX_FACTORS_REASON = "num_factors + 2 * use_bias columns of the factors-only handle"
    LOAD_CHECKS_MAX_FACTORS = False

    # what the device-scoring surface reads: as IALSRecommender
    mode = "user"
    score_contract = "mf"

    def __init__(self, URM_train, recompile_cython=False, algorithm_name="MF_BPR", device=0, verbose=False):
        super(_MatrixFactorization_Cython, self).__init__(URM_train)
        self._URM_eval = self.URM_train
        self.normalize = False
        self.algorithm_name = algorithm_name
        self.device = device
        self.verbose = verbose
        self.use_bias = False
        self.engine = None
        self.num_factors = None
        self.epochs_best = 0
        self.best_validation_metric = None
        self._model = None
        self._best = None
        self._stale = False      # the device state is newer than the members read back from it
        self.train_route = L.MF_SGD_AUTO      # L.MF_SGD_SEQUENTIAL / L.MF_SGD_LEVELLED: the route of every epoch (the same bytes either way)

    def _open(self, num_factors, use_bias):
        """the handle with num_factors + 2 use_bias columns; num_factors stays the model's"""
        columns = int(num_factors) + 2 * int(bool(use_bias))
        if int(num_factors) < 1 or columns > self.MAX_FACTORS:
            raise ValueError("{}: num_factors + 2 * use_bias must be in [1, {}] ({}), provided was num_factors {}, use_bias {}".format(
                self.RECOMMENDER_NAME, self.MAX_FACTORS, self.MAX_FACTORS_REASON, num_factors, use_bias))
        self._build(columns)
        self.num_factors = int(num_factors)
        self.use_bias = bool(use_bias)

    def fit(self, epochs=300, batch_size=1000, num_factors=10, positive_threshold_BPR=None, learning_rate=0.001, use_bias=True,
            sgd_mode='sgd', negative_interactions_quota=0.0, init_mean=0.0, init_std_dev=0.1, user_reg=0.0, item_reg=0.0, bias_reg=0.0,
            positive_reg=0.0, negative_reg=0.0, verbose=False, random_seed=None, **earlystopping_kwargs):
        if self.algorithm_name == "ASY_SVD":
            raise NotImplementedError(
                "{}: ASY_SVD is not implemented: the reference's batch update reads the profile bounds and the accumulated user vector of "
                "the last sample drawn in the batch's first phase, not of the sample being applied "
                "(MatrixFactorization_Cython_Epoch.pyx:541-576)".format(self.RECOMMENDER_NAME))
        if self.algorithm_name not in ALGORITHM_NAME_VALUES:
            raise ValueError("Value for 'algorithm_name' not recognized. Acceptable values are {}, provided was '{}'".format(
                ALGORITHM_NAME_VALUES, self.algorithm_name))
        if sgd_mode not in SGD_MODE_VALUES:
            raise ValueError("Value for 'sgd_mode' not recognized. Acceptable values are {}, provided was '{}'".format(SGD_MODE_VALUES, sgd_mode))
        assert negative_interactions_quota >= 0.0 and negative_interactions_quota < 1.0, \
            "{}: negative_interactions_quota must be a float value >=0 and < 1.0, provided was '{}'".format(
                self.RECOMMENDER_NAME, negative_interactions_quota)
        if not 1 <= int(batch_size) <= L.MF_SGD_MAX_BATCH:
            raise ValueError("{}: batch_size must be in [1, {}], provided was {}".format(self.RECOMMENDER_NAME, L.MF_SGD_MAX_BATCH, batch_size))
        bpr = self.algorithm_name == "MF_BPR"
        use_bias = bool(use_bias)

        # the matrix the samples come from (MatrixFactorization_Cython.py:62-104)
        URM_train_positive = self.URM_train.copy()
        if bpr and positive_threshold_BPR is not None:
            URM_train_positive.data = URM_train_positive.data >= positive_threshold_BPR
            URM_train_positive.eliminate_zeros()
            assert URM_train_positive.nnz > 0, "MatrixFactorization_Cython: URM_train_positive is empty, positive threshold is too high"
        profiles = sps.csr_matrix((np.array(URM_train_positive.data, dtype=np.float64), URM_train_positive.indices, URM_train_positive.indptr),
                                  shape=URM_train_positive.shape, copy=True)
        profiles.sum_duplicates()
        profiles.sort_indices()

        self._open(num_factors, use_bias)      # the engine with URM_train's seen mask
        self.sgd_mode = sgd_mode
        self.verbose = verbose
        self.positive_threshold_BPR = positive_threshold_BPR
        self.learning_rate = learning_rate
        self.negative_interactions_quota = negative_interactions_quota
        self.batch_size = int(batch_size)
        self.random_seed = random_seed

        # the epoch object's own draws (MatrixFactorization_Cython_Epoch.pyx:140-173)
        if random_seed is not None:
            np.random.seed(seed=random_seed)
        user_factors = np.random.normal(init_mean, init_std_dev, (self.n_users, self.num_factors)).astype(np.float64)
        item_factors = np.random.normal(init_mean, init_std_dev, (self.n_items, self.num_factors)).astype(np.float64)
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if random_seed is None else int(random_seed)

        # what each class's fit() forwards; everything else keeps the epoch object's default of 0
        rates = dict(learning_rate=float32_value(learning_rate), user_reg=float32_value(user_reg))
        if bpr:
            rates.update(positive_reg=float32_value(positive_reg), negative_reg=float32_value(negative_reg))
        else:
            rates.update(item_reg=float32_value(item_reg), bias_reg=float32_value(bias_reg),
                         negative_interactions_quota=float(negative_interactions_quota))
        self.engine.mf_sgd_init(self.algorithm_name, profiles, user_factors, item_factors, use_bias=use_bias, sgd_mode=sgd_mode, seed=seed,
                                **rates)
        self._prepare_model_for_validation()
        self._update_best_model()
        self._train_with_early_stopping(epochs, **earlystopping_kwargs)
        self._restore_best_model()

    # ---- the members: float64 read-backs ---------------------------------------------------------------
    def _member(self, name):
        self._require_engine()
        if self._model is None:
            raise RuntimeError("{}: model has no factors; call fit() or loadModel() first".format(self.RECOMMENDER_NAME))
        return self._model[name]

    USER_factors = property(lambda self: self._member("USER_factors"))
    ITEM_factors = property(lambda self: self._member("ITEM_factors"))
    USER_bias = property(lambda self: self._member("USER_bias"))
    ITEM_bias = property(lambda self: self._member("ITEM_bias"))
    GLOBAL_bias = property(lambda self: self._member("GLOBAL_bias"))

    @staticmethod
    def _as_members(params):
        out = {n: np.array(params[n], dtype=np.float64) for n in _MEMBERS}
        out["GLOBAL_bias"] = np.array(out["GLOBAL_bias"].ravel()[0])      # (get_GLOBAL_bias: a 0-d array)
        return out

    def _prepare_model_for_validation(self):
        """the current float64 state read back, and published to the tensors every score is formed from"""
        self._model = self._as_members(self.engine.mf_sgd_state()["params"])
        self.engine.mf_sgd_publish()
        self._stale = False

    def _update_best_model(self):
        """the best model: on the host as the reference keeps it, and in the handle's best slot (what fit() leaves to score with).
        Without validation the loop calls this once, behind the last epoch, whose state has not been read yet."""
        if self._stale:
            self._prepare_model_for_validation()
        self._best = {n: v.copy() for n, v in self._model.items()}
        self.engine.snapshot_best()

    USER_factors_best = property(lambda self: self._best["USER_factors"])
    ITEM_factors_best = property(lambda self: self._best["ITEM_factors"])
    USER_bias_best = property(lambda self: self._best["USER_bias"])
    ITEM_bias_best = property(lambda self: self._best["ITEM_bias"])
    GLOBAL_bias_best = property(lambda self: self._best["GLOBAL_bias"])

    def _restore_best_model(self):
        self._model = {n: v.copy() for n, v in self._best.items()}
        self.engine.restore_best()

    def _run_epoch(self, num_epoch):
        self.engine.mf_sgd_epochs(1, self.batch_size, route=self.train_route)
        self._stale = True

    # ---- persistence: BaseMatrixFactorizationRecommender.saveModel's layout, the biases included ------------------
    def saveModel(self, folder_path, file_name=None):
        import os
        self._require_engine()
        os.makedirs(folder_path, exist_ok=True)
        arrays = {"USER_factors": self.USER_factors, "ITEM_factors": self.ITEM_factors,
                  "_cold_user_mask": np.ediff1d(self._URM_eval.indptr) == 0}
        if self.use_bias:
            arrays.update(ITEM_bias=self.ITEM_bias, USER_bias=self.USER_bias, GLOBAL_bias=self.GLOBAL_bias)
        jsons = {"use_bias": self.use_bias}
        kinds = dict([(n, "np.ndarray") for n in arrays] + [(n, "json") for n in jsons])
        files = dict([(n, n + ".npy") for n in arrays] + [(n, n + ".json") for n in jsons])
        jsons["__DataIO_attribute_to_type_dict"] = kinds
        jsons["__DataIO_attribute_to_file_name"] = files
        with zipfile.ZipFile(self._zip_path(folder_path, file_name), "w", compression=zipfile.ZIP_DEFLATED) as z:
            for name, a in arrays.items():
                buf = io.BytesIO()
                np.save(buf, a, allow_pickle=False)
                z.writestr(name + ".npy", buf.getvalue())
            for name, obj in jsons.items():
                z.writestr(name + ".json", json.dumps(obj))

    def loadModel(self, folder_path, file_name=None):
        """FactorModelMixin.loadModel without its refusal of biased models: the biases become the two extra columns"""
        with zipfile.ZipFile(self._zip_path(folder_path, file_name)) as z:
            kinds = json.loads(z.read("__DataIO_attribute_to_type_dict.json").decode())
            files = json.loads(z.read("__DataIO_attribute_to_file_name.json").decode())
            data = {}
            for name, member in files.items():
                raw = z.read(member)
                data[name] = np.load(io.BytesIO(raw), allow_pickle=False) if kinds[name] == "np.ndarray" else json.loads(raw.decode())
        U, V = np.asarray(data["USER_factors"], dtype=np.float64), np.asarray(data["ITEM_factors"], dtype=np.float64)
        if U.ndim != 2 or V.ndim != 2 or U.shape[0] != self.n_users or V.shape[0] != self.n_items or U.shape[1] != V.shape[1]:
            raise ValueError("{}: saved factors are {} and {}, URM_train is {} x {}".format(
                self.RECOMMENDER_NAME, U.shape, V.shape, self.n_users, self.n_items))
        use_bias = bool(data.get("use_bias"))
        model = {"USER_factors": U, "ITEM_factors": V, "USER_bias": np.zeros(self.n_users), "ITEM_bias": np.zeros(self.n_items),
                 "GLOBAL_bias": np.array(0.0)}
        if use_bias:
            model["USER_bias"] = np.asarray(data["USER_bias"], dtype=np.float64).reshape(self.n_users)
            model["ITEM_bias"] = np.asarray(data["ITEM_bias"], dtype=np.float64).reshape(self.n_items)
            model["GLOBAL_bias"] = np.array(float(np.asarray(data["GLOBAL_bias"]).ravel()[0]))
        self._open(U.shape[1], use_bias)
        if use_bias:      # ganmf_mf_sgd_publish's layout
            ones_u, ones_i = np.ones((self.n_users, 1)), np.ones((self.n_items, 1))
            U = np.hstack([U, (model["USER_bias"] + model["GLOBAL_bias"])[:, None], ones_u])
            V = np.hstack([V, ones_i, model["ITEM_bias"][:, None]])
        self.engine.set_tensor(L.T_USER_EMB, U)
        self.engine.set_tensor(L.T_ITEM_EMB, V)
        self._model = model
        self._stale = False
        self._best = {n: v.copy() for n, v in model.items()}
        self.engine.snapshot_best()


class MatrixFactorization_BPR_Cython(_MatrixFactorization_Cython):
    """Subclass allowing only for MF BPR"""

    RECOMMENDER_NAME = "MatrixFactorization_BPR_Cython_Recommender"

    def __init__(self, *pos_args, **key_args):
        super(MatrixFactorization_BPR_Cython, self).__init__(*pos_args, algorithm_name="MF_BPR", **key_args)

    def fit(self, **key_args):
        key_args["use_bias"] = False
        key_args["negative_interactions_quota"] = 0.0
        super(MatrixFactorization_BPR_Cython, self).fit(**key_args)


class MatrixFactorization_FunkSVD_Cython(_MatrixFactorization_Cython):
    """Subclass allowing only for FunkSVD: R ~ U V^T (+ the three biases), the squared error on sampled entries by mini-batch SGD"""

    RECOMMENDER_NAME = "MatrixFactorization_FunkSVD_Cython_Recommender"

    def __init__(self, *pos_args, **key_args):
        super(MatrixFactorization_FunkSVD_Cython, self).__init__(*pos_args, algorithm_name="FUNK_SVD", **key_args)

    def fit(self, **key_args):
        super(MatrixFactorization_FunkSVD_Cython, self).fit(**key_args)


class MatrixFactorization_AsySVD_Cython(_MatrixFactorization_Cython):
    """Subclass for the asymmetric SVD model, which is not implemented: fit() raises NotImplementedError (module docstring)"""

    RECOMMENDER_NAME = "MatrixFactorization_AsySVD_Cython_Recommender"

    def __init__(self, *pos_args, **key_args):
        super(MatrixFactorization_AsySVD_Cython, self).__init__(*pos_args, algorithm_name="ASY_SVD", **key_args)

    def fit(self, **key_args):
        super(MatrixFactorization_AsySVD_Cython, self).fit(**key_args)
