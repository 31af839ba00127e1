from ganmf_amd import MF_SGD as _MF_SGD


class _MatrixFactorization_Cython(_MF_SGD._MatrixFactorization_Cython):
    """`MatrixFactorization.Cython.MatrixFactorization_Cython._MatrixFactorization_Cython` — the MI355X implementation under the
    reference's import path."""


class MatrixFactorization_BPR_Cython(_MF_SGD.MatrixFactorization_BPR_Cython):
    """`MatrixFactorization.Cython.MatrixFactorization_Cython.MatrixFactorization_BPR_Cython` — the MI355X implementation."""


class MatrixFactorization_FunkSVD_Cython(_MF_SGD.MatrixFactorization_FunkSVD_Cython):
    """`MatrixFactorization.Cython.MatrixFactorization_Cython.MatrixFactorization_FunkSVD_Cython` — the MI355X implementation."""


class MatrixFactorization_AsySVD_Cython(_MF_SGD.MatrixFactorization_AsySVD_Cython):
    """`MatrixFactorization.Cython.MatrixFactorization_Cython.MatrixFactorization_AsySVD_Cython` — fit() raises NotImplementedError."""
