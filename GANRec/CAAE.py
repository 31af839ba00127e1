from ganmf_amd.CAAE import CAAE as _CAAE


class CAAE(_CAAE):
    """`GANRec.CAAE.CAAE` — the MI355X implementation under the reference's import path."""
