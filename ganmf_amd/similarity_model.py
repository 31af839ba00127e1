"""What the similarity-matrix models computed by libganmf_hip.so share on the host -- the counterpart of FactorModelMixin for the
reference's BaseSimilarityMatrixRecommender family (Base/BaseSimilarityMatrixRecommender.py:16-92: scores = URM_train[users] . W_sparse):
the handle that holds a weighted URM and an item similarity matrix instead of tensors (GANMF_MODEL_ITEMSIM), W_sparse read from the
device, and persistence in the layout the reference's DataIO writes for {"W_sparse": ...} (Base/DataIO.py:103-183).  A class that uses
it provides RECOMMENDER_NAME, URM_train, n_users / n_items, device, _URM_eval and _reset_score_filter()."""
import io
import json
import os
import zipfile

import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .engine import Engine


class SimilarityModelMixin(object):
    # ---- engine plumbing -----------------------------------------------------------------------
    def _make_engine(self):
        """a similarity-matrix handle (GANMF_MODEL_ITEMSIM); num_factors, emb_dim and batch_size mean nothing to it"""
        return Engine(self.n_users, self.n_items, 1, 1, 1, model=L.MODEL_ITEMSIM, device=self.device)

    def _build(self):
        """A fresh engine that holds URM_train -- the matrix the scores are formed from, weighted if fit() weighted it -- in both
        orientations, in canonical form, and the seen mask."""
        if self.engine is not None:
            self.engine.close()
        urm = self._canonical(self.URM_train)
        self.engine = self._make_engine()
        self.engine.set_confidence(0, urm)
        self.engine.set_confidence(1, self._urm_by_item(urm))
        self.engine.set_seen(self._URM_eval)
        self._reset_score_filter()

    @staticmethod
    def _canonical(urm):
        """a float32 CSR copy with sorted indices and duplicates summed"""
        urm = sps.csr_matrix(urm, dtype=np.float32, copy=True)
        urm.sum_duplicates()
        urm.sort_indices()
        return urm

    @staticmethod
    def _urm_by_item(urm):
        """The canonical items x users CSR (float32, users ascending inside an item, duplicates summed) of a users x items matrix:
        what side 1 of the handle holds."""
        by_item = SimilarityModelMixin._canonical(urm).tocsc()
        by_item.sort_indices()
        return sps.csr_matrix((by_item.data, by_item.indices, by_item.indptr), shape=(urm.shape[1], urm.shape[0]))

    def _restore_side1(self):
        """side 1 back to URM_train's own values after a fit that put other values there (nothing reads it after the fit; kept
        consistent with side 0)"""
        self.engine.set_confidence(1, self._urm_by_item(self.URM_train))

    def _require_engine(self):
        if self.engine is None:
            raise RuntimeError("{}: model has no device state; call fit() or loadModel() first".format(self.RECOMMENDER_NAME))

    # ---- the similarity matrix (Base/BaseSimilarityMatrixRecommender.py:16-30) --------------------
    # item x item, scores = URM_train[users] . W_sparse; a user-based model (UserKNN.py) sets this to "user": user x user, scores =
    # W_sparse[users] . URM_train
    _similarity_of = "item"

    @property
    def W_sparse(self):
        """scipy CSR float32 [n_items, n_items], rows = neighbour, columns = item: the reference's layout (a user-based model:
        [n_users, n_users], row u = the users whose profiles user u's scores sum)"""
        self._require_engine()
        return self.engine.user_similarity() if self._similarity_of == "user" else self.engine.item_similarity()

    # ---- what a similarity-matrix model does not have ---------------------------------------------
    honours_items_to_compute = True

    def prediction_similarity(self, *args, **kwargs):
        raise NotImplementedError("{}: the prediction-similarity study is defined on factor models".format(self.RECOMMENDER_NAME))

    def recommend_candidates(self, *args, **kwargs):
        raise NotImplementedError("{}: candidate scoring gathers factor rows; rank with recommend(items_to_compute=...)".format(
            self.RECOMMENDER_NAME))

    def _device_ranking_args(self, user_id_array, cutoffs, max_cutoff, candidates_csr=None):
        """no candidate route on the device (it gathers factor rows): the candidate hooks return None and
        EvaluatorNegativeItemSampleFast takes its other route, recommend(items_to_compute=...)"""
        if candidates_csr is not None:
            return None
        return super(SimilarityModelMixin, self)._device_ranking_args(user_id_array, cutoffs, max_cutoff)

    # ---- persistence: the layout the reference's DataIO writes (Base/DataIO.py:103-183) ----------
    def _zip_path(self, folder_path, file_name):
        return os.path.join(folder_path, (self.RECOMMENDER_NAME if file_name is None else file_name) + ".zip")

    def saveModel(self, folder_path, file_name=None):
        self._require_engine()
        os.makedirs(folder_path, exist_ok=True)
        jsons = {"__DataIO_attribute_to_type_dict": {"W_sparse": "sps.spmatrix"},
                 "__DataIO_attribute_to_file_name": {"W_sparse": "W_sparse.npz"}}
        buf = io.BytesIO()
        sps.save_npz(buf, self.W_sparse)
        with zipfile.ZipFile(self._zip_path(folder_path, file_name), "w", compression=zipfile.ZIP_DEFLATED) as z:
            z.writestr("W_sparse.npz", buf.getvalue())
            for name, obj in jsons.items():
                z.writestr(name + ".json", json.dumps(obj))

    def loadModel(self, folder_path, file_name=None):
        """The saved W_sparse goes to the device; the scores are formed from this object's URM_train (as in the reference, whose
        saved model holds W_sparse only)."""
        with zipfile.ZipFile(self._zip_path(folder_path, file_name)) as z:
            kinds = json.loads(z.read("__DataIO_attribute_to_type_dict.json").decode())
            files = json.loads(z.read("__DataIO_attribute_to_file_name.json").decode())
            if kinds.get("W_sparse") != "sps.spmatrix":
                raise ValueError("{}: the saved model holds no sparse W_sparse".format(self.RECOMMENDER_NAME))
            W = sps.load_npz(io.BytesIO(z.read(files["W_sparse"])))
        n = self.n_users if self._similarity_of == "user" else self.n_items
        if W.shape != (n, n):
            raise ValueError("{}: the saved W_sparse is {}, URM_train has {} {}s".format(self.RECOMMENDER_NAME, W.shape, n, self._similarity_of))
        self._build()
        if self._similarity_of == "user":
            self.engine.set_user_similarity(W)
        else:
            self.engine.set_item_similarity(W)
