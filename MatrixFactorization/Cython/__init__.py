"""`MatrixFactorization.Cython`: the reference keeps its Cython epoch here; this repository's SGD matrix factorisations train on the
device instead.  The search path is extended as in the parent package."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
