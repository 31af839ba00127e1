// mf_sgd.hpp -- SGD matrix factorisation trained on the device: the MF_BPR and FUNK_SVD epochs of the reference's
// MatrixFactorization/Cython/MatrixFactorization_Cython_Epoch.pyx (:287-389, :614-696), its adaptive_gradient (:760-798) and its two
// samplers (:803-910), restated as HIP kernels.  float64 throughout, as the reference; floating-point contraction is off: every
// product and sum rounds once, as on the reference's x86-64 build.
//
// State.  W [n_users, k] and H [n_items, k] row-major, USER_bias [n_users], ITEM_bias [n_items], GLOBAL_bias [1], and two more arrays
// of every one of them: st0 the AdaGrad / RMSprop cache or Adam's first moment, st1 Adam's second moment, one value PER ELEMENT.
//
// A mini-batch is list[first, first + count) and has two phases.
//   Phase 1 (mf_predict_kernel, one launch): one wave per sample, parameters frozen.  Lane l adds the products of the factors
//     l, l + 64, ... in ascending order, then the 64 partial sums are added by the xor butterfly of mf_wave_sum (offsets 32, 16, ...,
//     1): x.  MF_BPR stores 1 / (1 + exp(x)) with x = sum W_u (H_i - H_j); FUNK_SVD stores rating - (((GLOBAL + USER_b[u]) +
//     ITEM_b[i]) + x) with x = sum W_u H_i (the biases only with use_bias) into terms[0, count).
//   The batch scalar s = mf_batch_mean(terms, count): lane l adds terms[l], terms[l + 64], ... ascending, the same butterfly, divided
//     by count.  Every wave that needs s forms it itself from the same buffer in the same order: the same bytes wherever it is formed.
//   Phase 2 (mf_update_kernel): the samples in list order, each reading the current rows.  One wave per sample, lane l owns the factors
//     l, l + 64, ...; lane 0 owns the two bias scalars of the sample; nothing crosses lanes.  Per factor (mf_apply):
//       MF_BPR:   g_i = s W_u - positive_reg H_i;  g_j = s (-W_u) - negative_reg H_j;  g_u = s (H_i - H_j) - user_reg W_u
//       FUNK_SVD: g_i = s W_u - positive_reg H_i;  g_u = s H_i - user_reg W_u      (the two biases first: g = s - bias_reg b)
//     each through sgd_adapt (sgd_adapt.hpp) with the element's own state, then x += lr g.  FUNK_SVD with use_bias updates GLOBAL_bias
//     once per batch in front of the samples (head != 0: lane 0 of the first wave).  Adam divides by 1 - the beta powers of the BATCH
//     (b1p, b2p: formed on the host by repeated multiplication, one per batch).
//
// Routes (mf_update_kernel).  walk = 1: ONE wave applies the batch in list order; an element is always read and written by the same
// lane, so program order is all the ordering there is.  walk = 0: wave w applies list[order[lvl_first + w]]; the caller launches one
// grid per level of level_sched.hpp, whose samples share no row.  Both routes run mf_apply, so they write the same bytes.  No atomics,
// no workgroup waits for another inside a kernel.
//
// Sampler: draw_kernel of counter_draw.hpp, which states the scheme in full.  MF_BPR draws the triple (rated = 0), FUNK_SVD one item
// with its rating (rated = 1).
//
// Publish (mf_publish_kernel): the float64 state rounded into the handle's float32 factor tensors; with use_bias two more columns,
// U' = [W | USER_b + GLOBAL | 1], V' = [H | 1 | ITEM_b], so that U' V'^T is W H^T + ITEM_b + GLOBAL + USER_b[u].
#pragma once
#include <hip/hip_runtime.h>
#include "counter_draw.hpp"
#include "sgd_adapt.hpp"

namespace ganmf {

constexpr int MF_SGD_WAVE = 64;
constexpr int MF_SGD_THREADS = 256;      // four samples per workgroup
enum MfSgdAlgo : int { MF_SGD_BPR = 0, MF_SGD_FUNK = 1, MF_SGD_ALGOS = 2 };

struct MfSgdP {
  double *W, *H, *ub, *ib, *gb;              // parameters
  double *W0, *H0, *ub0, *ib0, *gb0;         // st0 of each
  double *W1, *H1, *ub1, *ib1, *gb1;         // st1 of each
  int k, algo, use_bias, sgd;                // sgd: SgdMode
  double lr, user_reg, pos_reg, neg_reg, bias_reg, gamma, b1, b2;
  const int* users;                          // the sample list
  const int* pos;
  const int* neg;                            // MF_BPR only
  const double* rating;                      // FUNK_SVD only
  double* terms;                             // [batch] phase 1's per-sample terms
  const long long* order;                    // walk = 0: the list positions sorted by (batch, level)
};

__device__ __forceinline__ double mf_wave_sum(double v) {
#pragma clang fp contract(off)
  for (int o = MF_SGD_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, MF_SGD_WAVE);
  return v;
}

__device__ __forceinline__ double mf_batch_mean(const double* terms, long long count, int lane) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (long long q = lane; q < count; q += MF_SGD_WAVE) acc += terms[q];
  return mf_wave_sum(acc) / (double)count;
}

__global__ __launch_bounds__(MF_SGD_THREADS) void mf_predict_kernel(const MfSgdP p, long long first, long long count) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x % MF_SGD_WAVE;
  const long long w = (long long)blockIdx.x * (MF_SGD_THREADS / MF_SGD_WAVE) + threadIdx.x / MF_SGD_WAVE;
  if (w >= count) return;      // (a whole wave leaves: the shuffles below see 64 lanes)
  const long long t = first + w;
  const int u = p.users[t], i = p.pos[t];
  const double* Wu = p.W + (size_t)u * p.k;
  const double* Hi = p.H + (size_t)i * p.k;
  double acc = 0.0, term;
  if (p.algo == MF_SGD_BPR) {
    const double* Hj = p.H + (size_t)p.neg[t] * p.k;
    for (int f = lane; f < p.k; f += MF_SGD_WAVE) acc += Wu[f] * (Hi[f] - Hj[f]);
    const double x = mf_wave_sum(acc);
    term = 1.0 / (1.0 + exp(x));
  } else {
    for (int f = lane; f < p.k; f += MF_SGD_WAVE) acc += Wu[f] * Hi[f];
    const double x = mf_wave_sum(acc);
    const double prediction = p.use_bias ? ((p.gb[0] + p.ub[u]) + p.ib[i]) + x : x;
    term = p.rating[t] - prediction;
  }
  if (lane == 0) p.terms[w] = term;
}

// GLOBAL_bias, once per batch (:338-347); lane 0 of one wave
__device__ __forceinline__ void mf_global_bias(const MfSgdP& p, double s, double b1p, double b2p) {
#pragma clang fp contract(off)
  double g = s - p.bias_reg * p.gb[0];
  g = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, g, p.gb0, p.gb1, b1p, b2p);
  p.gb[0] = p.gb[0] + p.lr * g;
}

// one sample, one wave
__device__ __forceinline__ void mf_apply(const MfSgdP& p, long long t, double s, double b1p, double b2p, int lane) {
#pragma clang fp contract(off)
  const int u = p.users[t], i = p.pos[t], k = p.k;
  const size_t ru = (size_t)u * k, ri = (size_t)i * k;
  if (p.algo == MF_SGD_BPR) {
    const size_t rj = (size_t)p.neg[t] * k;
    for (int f = lane; f < k; f += MF_SGD_WAVE) {
      const double Hi = p.H[ri + f], Hj = p.H[rj + f], Wu = p.W[ru + f];
      double gi = s * Wu - p.pos_reg * Hi;
      double gj = s * (-Wu) - p.neg_reg * Hj;
      double gu = s * (Hi - Hj) - p.user_reg * Wu;
      gi = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gi, p.H0 + ri + f, p.H1 + ri + f, b1p, b2p);
      gj = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gj, p.H0 + rj + f, p.H1 + rj + f, b1p, b2p);
      gu = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gu, p.W0 + ru + f, p.W1 + ru + f, b1p, b2p);
      p.W[ru + f] = Wu + p.lr * gu;
      p.H[ri + f] = Hi + p.lr * gi;
      p.H[rj + f] = Hj + p.lr * gj;
    }
    return;
  }
  if (p.use_bias && lane == 0) {
    double gbi = s - p.bias_reg * p.ib[i];
    double gbu = s - p.bias_reg * p.ub[u];
    gbi = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gbi, p.ib0 + i, p.ib1 + i, b1p, b2p);
    gbu = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gbu, p.ub0 + u, p.ub1 + u, b1p, b2p);
    p.ib[i] = p.ib[i] + p.lr * gbi;
    p.ub[u] = p.ub[u] + p.lr * gbu;
  }
  for (int f = lane; f < k; f += MF_SGD_WAVE) {
    const double Hi = p.H[ri + f], Wu = p.W[ru + f];
    double gi = s * Wu - p.pos_reg * Hi;
    double gu = s * Hi - p.user_reg * Wu;
    gi = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gi, p.H0 + ri + f, p.H1 + ri + f, b1p, b2p);
    gu = sgd_adapt(p.sgd, p.gamma, p.b1, p.b2, gu, p.W0 + ru + f, p.W1 + ru + f, b1p, b2p);
    p.H[ri + f] = Hi + p.lr * gi;
    p.W[ru + f] = Wu + p.lr * gu;
  }
}

// the batch list[first, first + count).  walk = 1: launched with ONE wave, which applies all of it in order.  walk = 0: wave w of the
// grid applies list[order[lvl_first + w]], w < lvl_count (one level of the batch).  head != 0: this launch is the batch's first one and
// carries the GLOBAL_bias update.
__global__ __launch_bounds__(MF_SGD_THREADS) void mf_update_kernel(const MfSgdP p, long long first, long long count, long long lvl_first,
                                                                   long long lvl_count, int walk, int head, double b1p, double b2p) {
  const int lane = threadIdx.x % MF_SGD_WAVE;
  const long long w = (long long)blockIdx.x * (blockDim.x / MF_SGD_WAVE) + threadIdx.x / MF_SGD_WAVE;
  if (walk ? w != 0 : w >= lvl_count) return;
  const double s = mf_batch_mean(p.terms, count, lane);
  if (head && w == 0 && lane == 0 && p.algo == MF_SGD_FUNK && p.use_bias) mf_global_bias(p, s, b1p, b2p);
  if (walk) {
    for (long long t = first; t < first + count; ++t) mf_apply(p, t, s, b1p, b2p, lane);
  } else {
    mf_apply(p, p.order[lvl_first + w], s, b1p, b2p, lane);
  }
}

// ---- publish ----------------------------------------------------------------------------------------------------------------------
struct MfPublishP {
  const double *W, *H, *ub, *ib, *gb;
  float* Ue;                   // [n_users, ld] the handle's factor tensors, k + 2 use_bias columns in use
  float* V;                    // [n_items, ld]
  int n_users, n_items, k, use_bias, ld;
};

__global__ __launch_bounds__(MF_SGD_THREADS) void mf_publish_kernel(const MfPublishP p) {
#pragma clang fp contract(off)
  const int cols = p.k + 2 * p.use_bias;
  const long long g = (long long)blockIdx.x * MF_SGD_THREADS + threadIdx.x;
  if (g >= ((long long)p.n_users + p.n_items) * cols) return;
  const long long row = g / cols;
  const int c = (int)(g % cols);
  if (row < p.n_users) {
    const double v = c < p.k ? p.W[(size_t)row * p.k + c] : c == p.k ? p.ub[row] + p.gb[0] : 1.0;
    p.Ue[(size_t)row * p.ld + c] = (float)v;
  } else {
    const long long r = row - p.n_users;
    const double v = c < p.k ? p.H[(size_t)r * p.k + c] : c == p.k ? 1.0 : p.ib[r];
    p.V[(size_t)r * p.ld + c] = (float)v;
  }
}

}  // namespace ganmf
