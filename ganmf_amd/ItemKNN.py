"""ItemKNNCFRecommender -- item-based collaborative filtering, host mirror of the reference class (KNN/ItemKNNCFRecommender.py:18-54;
the neighbourhood family of the comparison table in RecSysExp.py:71-97).

Same constructor, fit() keyword arguments, W_sparse layout and saved-model layout as the reference, so it can stand in for
`KNN.ItemKNNCFRecommender.ItemKNNCFRecommender` under RecSysExp.py / RunBestParameters.py.  The similarity matrix is computed by
libganmf_hip.so (ganmf_itemknn_fit: the dot products of every item with every other, the similarity's denominator and the top-K
selection, HIP kernels on gfx950, on a GANMF_MODEL_ITEMSIM handle) and stays on the device, where scoring -- URM_train[users] .
W_sparse as a sparse product -- recommendation and evaluation run through the routes of DeviceScoringMixin.  This file holds what the
reference decides on the host: the feature weighting, which similarities binarise the data and switch `normalize` off, and the
per-item terms of the denominators (Base/Similarity/Compute_Similarity_Python.py:51-107, 233-250)."""
from .knn_model import TF_IDF, NeighbourhoodCFRecommender, okapi_BM_25      # (the weightings: part of this module's surface)


class ItemKNNCFRecommender(NeighbourhoodCFRecommender):
    """ ItemKNN recommender"""

    RECOMMENDER_NAME = "ItemKNNCFRecommender"

    _fit_side = 1      # the similarity compares the columns of URM_train: side 1 of the handle, the per-item terms
    _target = "item"

    # ---- fit (ItemKNNCFRecommender.py:31-54): knn_model.NeighbourhoodCFRecommender.fit -------------
    def _device_fit(self, kind, topk, **kw):
        self.engine.itemknn_fit(kind, topk, **kw)
