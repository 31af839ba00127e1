"""What the factor models computed by libganmf_hip.so share on the host (IALSRecommender, PureSVDRecommender): the factors-only
handle (GANMF_MODEL_MF), USER_factors / ITEM_factors read from the device, and persistence in the layout the reference's DataIO
writes (Base/DataIO.py:103-183).  A class that uses it provides RECOMMENDER_NAME, MAX_FACTORS, MAX_FACTORS_REASON, n_users / n_items, device, use_bias,
_URM_eval, _reset_score_filter() and _update_best_model()."""
import io
import json
import os
import zipfile

import numpy as np

from . import _lib as L
from .engine import Engine


class FactorModelMixin(object):
    # ---- engine plumbing -----------------------------------------------------------------------
    def _make_engine(self, num_factors):
        """a factors-only handle (GANMF_MODEL_MF); emb_dim and batch_size mean nothing to it"""
        return Engine(self.n_users, self.n_items, num_factors, 1, 1, model=L.MODEL_MF, device=self.device)

    # MAX_FACTORS bounds what the class's own fit() can compute, for the reason MAX_FACTORS_REASON gives; scoring a loaded model has no
    # such bound, so a class whose limit is fit()'s alone sets LOAD_CHECKS_MAX_FACTORS = False
    LOAD_CHECKS_MAX_FACTORS = True

    def _build(self, num_factors, limit=True):
        if int(num_factors) < 1 or (limit and int(num_factors) > self.MAX_FACTORS):
            raise ValueError("{}: num_factors must be in [1, {}] ({}), provided was "
                             "{}".format(self.RECOMMENDER_NAME, self.MAX_FACTORS, self.MAX_FACTORS_REASON, num_factors))
        self.num_factors = int(num_factors)
        if self.engine is not None:
            self.engine.close()
        self.engine = self._make_engine(self.num_factors)
        self.engine.set_seen(self._URM_eval)
        self._reset_score_filter()

    def _require_engine(self):
        if self.engine is None:
            raise RuntimeError("{}: model has no device state; call fit() or loadModel() first".format(self.RECOMMENDER_NAME))

    # ---- factors (Base/BaseMatrixFactorizationRecommender.py:94-143) -----------------------------
    @property
    def USER_factors(self):
        self._require_engine()
        return self.engine.get_tensor(L.T_USER_EMB)

    @property
    def ITEM_factors(self):
        self._require_engine()
        return self.engine.get_tensor(L.T_ITEM_EMB)

    # ---- persistence: the layout the reference's DataIO writes (Base/DataIO.py:103-183) ----------
    def _zip_path(self, folder_path, file_name):
        return os.path.join(folder_path, (self.RECOMMENDER_NAME if file_name is None else file_name) + ".zip")

    def saveModel(self, folder_path, file_name=None):
        self._require_engine()
        os.makedirs(folder_path, exist_ok=True)
        arrays = {"USER_factors": self.USER_factors, "ITEM_factors": self.ITEM_factors,
                  "_cold_user_mask": np.ediff1d(self._URM_eval.indptr) == 0}
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
        with zipfile.ZipFile(self._zip_path(folder_path, file_name)) as z:
            kinds = json.loads(z.read("__DataIO_attribute_to_type_dict.json").decode())
            files = json.loads(z.read("__DataIO_attribute_to_file_name.json").decode())
            data = {}
            for name, member in files.items():
                raw = z.read(member)
                data[name] = np.load(io.BytesIO(raw), allow_pickle=False) if kinds[name] == "np.ndarray" else json.loads(raw.decode())
        if data.get("use_bias"):
            raise ValueError("{}: a saved model with biases is not supported".format(self.RECOMMENDER_NAME))
        U, V = np.asarray(data["USER_factors"]), np.asarray(data["ITEM_factors"])
        if U.shape[0] != self.n_users or V.shape[0] != self.n_items or U.shape[1] != V.shape[1]:
            raise ValueError("{}: saved factors are {} and {}, URM_train is {} x {}".format(
                self.RECOMMENDER_NAME, U.shape, V.shape, self.n_users, self.n_items))
        self._build(U.shape[1], limit=self.LOAD_CHECKS_MAX_FACTORS)
        self.engine.set_tensor(L.T_USER_EMB, U)
        self.engine.set_tensor(L.T_ITEM_EMB, V)
        self._update_best_model()
