from ganmf_amd.CFGAN import CFGAN as _CFGAN


class CFGAN(_CFGAN):
    """`GANRec.CFGAN.CFGAN` — the MI355X implementation under the reference's import path."""
