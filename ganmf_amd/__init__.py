"""ganmf_amd — MI355X-native GANMF / DisGANMF training hot path.

Python host mirror of the reference's recommender interface (GANRec/GANMF.py,
GANRec/DisGANMF.py) over the C ABI of libganmf_hip.so (include/ganmf_hip.h).  There is no CPU
fallback: without the HIP library and a GPU the classes raise.
"""
from ._lib import build_library, library_path, load_library  # noqa: F401

__all__ = ["build_library", "library_path", "load_library", "GANMF", "DisGANMF", "CFGAN", "CAAE", "IALSRecommender", "PureSVDRecommender",
           "NMFRecommender"]


def __getattr__(name):
    if name == "GANMF":
        from .GANMF import GANMF
        return GANMF
    if name == "DisGANMF":
        from .DisGANMF import DisGANMF
        return DisGANMF
    if name == "CFGAN":
        from .CFGAN import CFGAN
        return CFGAN
    if name == "CAAE":
        from .CAAE import CAAE
        return CAAE
    if name == "IALSRecommender":
        from .IALS import IALSRecommender
        return IALSRecommender
    if name == "PureSVDRecommender":
        from .PureSVD import PureSVDRecommender
        return PureSVDRecommender
    if name == "NMFRecommender":
        from .NMF import NMFRecommender
        return NMFRecommender
    raise AttributeError(name)
