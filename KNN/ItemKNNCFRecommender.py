from ganmf_amd.ItemKNN import ItemKNNCFRecommender as _ItemKNNCFRecommender


class ItemKNNCFRecommender(_ItemKNNCFRecommender):
    """`KNN.ItemKNNCFRecommender.ItemKNNCFRecommender` — the MI355X implementation under the reference's import path."""
