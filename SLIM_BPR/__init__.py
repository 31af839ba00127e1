"""Drop-in package name for the SLIM recommenders this repository implements.

The reference's drivers import `SLIM_BPR.Cython.SLIM_BPR_Cython.SLIM_BPR_Cython` (RecSysExp.py, RunBestParameters.py).  As `KNN/`,
`GraphBased/`, `GANRec/` and `MatrixFactorization/` do, this package extends its search path with every other `SLIM_BPR/` directory
on `sys.path`: the module resolves here (first entry), any other submodule in the reference's directory."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
