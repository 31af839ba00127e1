from ganmf_amd.IALS import IALSRecommender as _IALSRecommender


class IALSRecommender(_IALSRecommender):
    """`MatrixFactorization.IALSRecommender.IALSRecommender` — the MI355X implementation under the reference's import path."""
