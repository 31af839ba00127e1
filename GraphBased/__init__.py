"""Drop-in package name for the graph-based recommenders this repository implements.

The reference's drivers import `GraphBased.P3alphaRecommender.P3alphaRecommender` and `GraphBased.RP3betaRecommender.RP3betaRecommender`
(RecSysExp.py, RunBestParameters.py).  As `KNN/`, `GANRec/` and `MatrixFactorization/` do, this package extends its search path with
every other `GraphBased/` directory on `sys.path`: the two modules resolve here (first entry), any other submodule in the reference's
directory."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
