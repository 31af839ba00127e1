from ganmf_amd.NMF import NMFRecommender as _NMFRecommender


class NMFRecommender(_NMFRecommender):
    """`MatrixFactorization.NMFRecommender.NMFRecommender` — the MI355X implementation under the reference's import path."""
