from ganmf_amd.P3 import RP3betaRecommender as _RP3betaRecommender


class RP3betaRecommender(_RP3betaRecommender):
    """`GraphBased.RP3betaRecommender.RP3betaRecommender` — the MI355X implementation under the reference's import path."""
