"""Drop-in package name for the matrix-factorisation recommenders this repository implements.

The reference's drivers import `MatrixFactorization.IALSRecommender.IALSRecommender`,
`MatrixFactorization.PureSVDRecommender.PureSVDRecommender` and `MatrixFactorization.NMFRecommender.NMFRecommender` next to other modules of the same package (the Cython models;
RecSysExp.py, RunBestParameters.py), which live only in the reference tree.  As `GANRec/` does, this package therefore extends its
search path with every other `MatrixFactorization/` directory on `sys.path`: `MatrixFactorization.IALSRecommender`,
`MatrixFactorization.PureSVDRecommender` and `MatrixFactorization.NMFRecommender` resolve here (first entry), every other submodule in the reference's directory."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
