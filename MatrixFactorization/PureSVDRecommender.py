from ganmf_amd.PureSVD import PureSVDRecommender as _PureSVDRecommender


class PureSVDRecommender(_PureSVDRecommender):
    """`MatrixFactorization.PureSVDRecommender.PureSVDRecommender` — the MI355X implementation under the reference's import path."""
