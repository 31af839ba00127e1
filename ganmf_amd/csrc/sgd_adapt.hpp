// sgd_adapt.hpp -- the adaptive gradient of the SGD trainers (slim_bpr.hpp, mf_sgd.hpp): the reference's adaptive_gradient
// (MatrixFactorization_Cython_Epoch.pyx:760-798; SLIM_BPR_Cython_Epoch.pyx:300-347 writes the same expressions out) on ONE state entry.
// st0 is the AdaGrad / RMSprop cache or Adam's first moment, st1 Adam's second moment; b1p and b2p are the beta powers Adam divides by
// (the caller's: SLIM-BPR's advance per sample, MF's per batch).  Floating-point contraction is off: every product and sum rounds once.
#pragma once
#include <hip/hip_runtime.h>

namespace ganmf {

enum SgdMode : int { SGD_PLAIN = 0, SGD_ADAGRAD = 1, SGD_RMSPROP = 2, SGD_ADAM = 3, SGD_MODES = 4 };

// updates the entry's state with the gradient g and returns the step
__device__ __forceinline__ double sgd_adapt(int mode, double gamma, double b1, double b2, double g, double* c0, double* c1, double b1p,
                                            double b2p) {
#pragma clang fp contract(off)
  if (mode == SGD_ADAGRAD) {
    const double c = *c0 + g * g;
    *c0 = c;
    return g / (sqrt(c) + 1e-8);
  }
  if (mode == SGD_RMSPROP) {
    const double c = *c0 * gamma + (1.0 - gamma) * (g * g);
    *c0 = c;
    return g / (sqrt(c) + 1e-8);
  }
  if (mode == SGD_ADAM) {
    const double m1 = *c0 * b1 + (1.0 - b1) * g;
    const double m2 = *c1 * b2 + (1.0 - b2) * (g * g);
    *c0 = m1;
    *c1 = m2;
    const double h1 = m1 / (1.0 - b1p);
    const double h2 = m2 / (1.0 - b2p);
    return h1 / (sqrt(h2) + 1e-8);
  }
  return g;
}

}  // namespace ganmf
