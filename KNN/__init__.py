"""Drop-in package name for the neighbourhood recommenders this repository implements.

The reference's drivers import `KNN.ItemKNNCFRecommender.ItemKNNCFRecommender` and `KNN.UserKNNCFRecommender.UserKNNCFRecommender`
next to other modules of the same package (the content-based and hybrid models; RecSysExp.py, RunBestParameters.py), which live only
in the reference tree.  As `GANRec/` and `MatrixFactorization/` do, this package therefore extends its search path with every other
`KNN/` directory on `sys.path`: `KNN.ItemKNNCFRecommender` and `KNN.UserKNNCFRecommender` resolve here (first entry), every other
submodule in the reference's directory."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
