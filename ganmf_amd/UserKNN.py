"""UserKNNCFRecommender -- user-based collaborative filtering, host mirror of the reference class (KNN/UserKNNCFRecommender.py:18-61;
the neighbourhood family of the comparison table in RecSysExp.py:71-97).

Same constructor, fit() keyword arguments, W_sparse layout ([n_users, n_users]) and saved-model layout as the reference, so it can stand
in for `KNN.UserKNNCFRecommender.UserKNNCFRecommender` under RecSysExp.py / RunBestParameters.py.  The reference computes the similarity
of URM_train.T: every per-item term of the item model becomes a per-user term (row norms, row counts).  The matrix is computed by
libganmf_hip.so (ganmf_userknn_fit: the row builder and selection of the item model reading side 0 of the handle instead of side 1,
then turned into rows) and stays on the device, where scoring -- W_sparse[users] . URM_train, a weighted sum of the neighbours' profile
rows (userknn_score_kernel) -- recommendation and evaluation run through the routes of DeviceScoringMixin.  What the reference decides
on the host is shared with ItemKNNCFRecommender: knn_model.py."""
import numpy as np

from .knn_model import NeighbourhoodCFRecommender


class UserKNNCFRecommender(NeighbourhoodCFRecommender):
    """ UserKNN recommender"""

    RECOMMENDER_NAME = "UserKNNCFRecommender"

    _fit_side = 0      # the similarity compares the rows of URM_train: side 0 of the handle, the per-user terms
    _target = "user"
    _similarity_of = "user"

    def __init__(self, URM_train, device=0, verbose=False):
        super(UserKNNCFRecommender, self).__init__(URM_train, device=device, verbose=verbose)
        cold_user_mask = np.ediff1d(self.URM_train.indptr) == 0
        if verbose and cold_user_mask.any():      # (UserKNNCFRecommender.py:31-35)
            print("{}: Detected {} ({:.2f} %) cold users.".format(
                self.RECOMMENDER_NAME, cold_user_mask.sum(), cold_user_mask.sum() / len(cold_user_mask) * 100))

    # ---- fit (UserKNNCFRecommender.py:39-61): knn_model.NeighbourhoodCFRecommender.fit; a binarising similarity puts its ones into
    # side 0, which is back at URM_train's values before fit() returns ----
    def _device_fit(self, kind, topk, **kw):
        self.engine.userknn_fit(kind, topk, **kw)
