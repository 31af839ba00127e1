"""`SLIM_BPR.Cython`: the reference keeps its Cython epoch here; this repository's SLIM_BPR_Cython trains on the device instead.
The search path is extended as in the parent package."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
