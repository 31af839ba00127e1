from ganmf_amd.UserKNN import UserKNNCFRecommender as _UserKNNCFRecommender


class UserKNNCFRecommender(_UserKNNCFRecommender):
    """`KNN.UserKNNCFRecommender.UserKNNCFRecommender` — the MI355X implementation under the reference's import path."""
