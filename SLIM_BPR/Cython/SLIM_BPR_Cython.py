from ganmf_amd.SLIM_BPR import SLIM_BPR_Cython as _SLIM_BPR_Cython


class SLIM_BPR_Cython(_SLIM_BPR_Cython):
    """`SLIM_BPR.Cython.SLIM_BPR_Cython.SLIM_BPR_Cython` — the MI355X implementation under the reference's import path."""
