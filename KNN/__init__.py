"""Drop-in package name for the neighbourhood recommenders this repository implements.

The reference's drivers import `KNN.ItemKNNCFRecommender.ItemKNNCFRecommender` next to other modules of the same package (the
user-based and content-based models; RecSysExp.py, RunBestParameters.py), which live only in the reference tree.  As `GANRec/` and
`MatrixFactorization/` do, this package therefore extends its search path with every other `KNN/` directory on `sys.path`:
`KNN.ItemKNNCFRecommender` resolves here (first entry), every other submodule in the reference's directory."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
