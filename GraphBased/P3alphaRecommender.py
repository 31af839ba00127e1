from ganmf_amd.P3 import P3alphaRecommender as _P3alphaRecommender


class P3alphaRecommender(_P3alphaRecommender):
    """`GraphBased.P3alphaRecommender.P3alphaRecommender` — the MI355X implementation under the reference's import path."""
