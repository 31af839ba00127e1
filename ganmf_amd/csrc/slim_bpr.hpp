// slim_bpr.hpp -- SLIM-BPR trained on the device: the epoch of the reference's SLIM_BPR/Cython/SLIM_BPR_Cython_Epoch.pyx:198-347 (dense
// and symmetric storage), its sampler (:427-471) and get_S (:373-421), restated as HIP kernels.  float64 throughout, as the reference.
//
// Storage.  S is [n, n] row-major, or -- symmetric -- one cell per unordered pair: cell(a, b) = S[r (r + 1) / 2 + c] with
// r = max(a, b), c = min(a, b) (the reference's Triangular_Matrix).  The optimiser state is two [n] vectors: st0 the AdaGrad / RMSprop
// cache or Adam's first moment, st1 Adam's second moment.
//
// One sample (u, i, j), one workgroup of SLIM_THREADS threads (slim_sample):
//   x = sum over the profile of u of cell(i, s) - cell(j, s): thread t adds the entries t, t + 256, ... of the profile in ascending
//       order, then the 256 partial sums are added by a fixed binary tree in LDS.  The same bytes on every run.
//   g = 1 / (1 + exp(x)); thread 0 updates the state of i and j and forms the step `upd` (sgd: g; adagrad / rmsprop: g / (sqrt(c_i) +
//       1e-8); adam: the bias-corrected moments of i ONLY, with the beta powers of this sample, pows[2 t], pows[2 t + 1], formed on
//       the host by repeated multiplication): the expressions of sgd_adapt.hpp, written out for the two entries together.
//   every s of the profile, one thread each: s != i: cell(i, s) += lr (upd - li cell(i, s));  s != j: cell(j, s) -= lr (upd - lj cell(j, s)).
//   No two of these touch one cell, with one exception: symmetric storage and a list that names a j INSIDE the profile (the sampler
//   never does; an injected list may): cell(i, j) is then written at s = j and at s = i.  Thread 0 applies that pair alone, in the
//   order of s, as the reference's loop over the ascending profile does.
//   Floating-point contraction is off: every product and sum rounds once, as on the reference's x86-64 build.
//
// Routes (slim_update_kernel).  walk = 1: ONE workgroup applies list[first, first + count) in order, a barrier between samples.
// walk = 0: workgroup b applies list[order[first + b]]; the caller launches one grid per level of level_sched.hpp, whose samples
// share no item.  Both routes run slim_sample, so they write the same bytes.  No workgroup waits for another inside a kernel.
//
// Sampler: draw_kernel of counter_draw.hpp, which states the scheme in full; SLIM-BPR draws the triple (rated = 0), num_users + 1
// samples per epoch.
//
// get_S (slim_rows_kernel): one workgroup per row; the row is copied (from the triangle when symmetric) into a private float64 row,
// its diagonal entry zero, and the topk largest are selected in float64 by select_topk_nonzero<double> (topk_rounds.hpp: arg-max
// rounds with ties to the smaller id); the non-zero picks are rounded to float32 and stored in the layout itemknn_pack_kernel reads.
#pragma once
#include <hip/hip_runtime.h>
#include "counter_draw.hpp"
#include "itemknn_rows.hpp"
#include "sgd_adapt.hpp"

namespace ganmf {

constexpr int SLIM_THREADS = 256;
static_assert(SLIM_THREADS == TOPK_THREADS, "slim_rows_kernel selects with the rounds of topk_rounds.hpp");

struct SlimP {
  const long long* indptr;     // the profiles: users x items, items ascending without repeats inside a user
  const int* items;
  double* S;
  double* st0;
  double* st1;
  int n_items, symmetric, sgd;      // sgd: SgdMode
  double lr, li, lj, gamma, b1, b2;
  const int* users;            // the sample list
  const int* pos;
  const int* neg;
  const double* pows;          // adam: [2 n] beta_1^t', beta_2^t' of every sample; else null
  const long long* order;      // walk = 0: the samples sorted by level
};

__host__ __device__ __forceinline__ size_t slim_cell(int symmetric, int n, int a, int b) {
  if (symmetric) {
    const size_t r = (size_t)(a > b ? a : b), c = (size_t)(a > b ? b : a);
    return r * (r + 1) / 2 + c;
  }
  return (size_t)a * (size_t)n + (size_t)b;
}

__device__ __forceinline__ void slim_sample(const SlimP& p, long long t, double* red, double* sh_upd) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int u = p.users[t], i = p.pos[t], j = p.neg[t];
  const long long a = p.indptr[u], b = p.indptr[u + 1];
  const int n = p.n_items, sym = p.symmetric;
  double acc = 0.0;
  for (long long q = a + tid; q < b; q += SLIM_THREADS) {
    const int s = p.items[q];
    acc += p.S[slim_cell(sym, n, i, s)] - p.S[slim_cell(sym, n, j, s)];
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = SLIM_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double x = red[0];
    const double g = 1.0 / (1.0 + exp(x));
    // sgd_adapt's expressions (sgd_adapt.hpp) written out for the PAIR of entries i and j: one test of the mode serves both, j's step
    // is never formed, and the beta powers are read inside the adam branch.  Two calls of sgd_adapt leave the same bytes and cost the
    // sequential walk 3 - 8 % (profiles/sgd_shared.md): this section stands between two barriers of every sample.
    double upd = g;
    if (p.sgd == SGD_ADAGRAD) {
      const double ci = p.st0[i] + g * g;
      p.st0[i] = ci;
      p.st0[j] = p.st0[j] + g * g;
      upd = g / (sqrt(ci) + 1e-8);
    } else if (p.sgd == SGD_RMSPROP) {
      const double ci = p.st0[i] * p.gamma + (1.0 - p.gamma) * (g * g);
      p.st0[i] = ci;
      p.st0[j] = p.st0[j] * p.gamma + (1.0 - p.gamma) * (g * g);
      upd = g / (sqrt(ci) + 1e-8);
    } else if (p.sgd == SGD_ADAM) {
      const double m1 = p.st0[i] * p.b1 + (1.0 - p.b1) * g;
      const double m2 = p.st1[i] * p.b2 + (1.0 - p.b2) * (g * g);
      p.st0[i] = m1;
      p.st1[i] = m2;
      const double h1 = m1 / (1.0 - p.pows[2 * t]);
      const double h2 = m2 / (1.0 - p.pows[2 * t + 1]);
      upd = h1 / (sqrt(h2) + 1e-8);
      p.st0[j] = p.st0[j] * p.b1 + (1.0 - p.b1) * g;
      p.st1[j] = p.st1[j] * p.b2 + (1.0 - p.b2) * (g * g);
    }
    *sh_upd = upd;
  }
  __syncthreads();
  const double upd = *sh_upd;
  // symmetric storage and both i and j inside the profile: cell(i, j) is written twice, by thread 0 below
  const bool pair = sym && in_profile(p.items, a, b, j) && in_profile(p.items, a, b, i);
  for (long long q = a + tid; q < b; q += SLIM_THREADS) {
    const int s = p.items[q];
    if (s != i && !(pair && s == j)) {
      double* c = p.S + slim_cell(sym, n, i, s);
      const double v = *c;
      *c = v + p.lr * (upd - p.li * v);
    }
    if (s != j && !(pair && s == i)) {
      double* c = p.S + slim_cell(sym, n, j, s);
      const double v = *c;
      *c = v - p.lr * (upd - p.lj * v);
    }
  }
  if (pair && tid == 0) {
    double* c = p.S + slim_cell(sym, n, i, j);
    double v = *c;
    if (j < i) {      // s = j comes first: the i update, then (s = i) the j update
      v = v + p.lr * (upd - p.li * v);
      v = v - p.lr * (upd - p.lj * v);
    } else {
      v = v - p.lr * (upd - p.lj * v);
      v = v + p.lr * (upd - p.li * v);
    }
    *c = v;
  }
}

__global__ __launch_bounds__(SLIM_THREADS) void slim_update_kernel(const SlimP p, long long first, long long count, int walk) {
  __shared__ double red[SLIM_THREADS];
  __shared__ double sh_upd;
  if (walk) {
    if (blockIdx.x != 0) return;
    for (long long t = first; t < first + count; ++t) {
      slim_sample(p, t, red, &sh_upd);
      __syncthreads();      // this sample's cells and state are written before the next one reads them
    }
  } else {
    if ((long long)blockIdx.x >= count) return;
    slim_sample(p, p.order[first + blockIdx.x], red, &sh_upd);
  }
}

// ---- get_S: the diagonal, and the top-k of every row in float64 ---------------------------------------------------------------------
__global__ __launch_bounds__(SLIM_THREADS) void slim_zero_diag_kernel(double* S, int n, int symmetric) {
  const int i = blockIdx.x * SLIM_THREADS + threadIdx.x;
  if (i < n) S[slim_cell(symmetric, n, i, i)] = 0.0;
}

struct SlimRowP {
  const double* S;
  int n_items, symmetric, topk;      // topk <= min(KNN_MAX_TOPK, n_items)
  double* rows;                      // [gridDim.x, n_items] a private row per workgroup
  int* out_idx;                      // [n_items, topk] picks in descending order of value
  float* out_val;
  int* out_cnt;                      // [n_items] stored picks (the non-zero ones)
};

__global__ __launch_bounds__(SLIM_THREADS) void slim_rows_kernel(const SlimRowP p) {
  __shared__ double wv[SLIM_THREADS / 64];
  __shared__ int wi[SLIM_THREADS / 64];
  __shared__ int s_stop;
  const int tid = threadIdx.x, n = p.n_items;
  double* w = p.rows + (size_t)blockIdx.x * n;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    int neg = 0;
    for (int j = tid; j < n; j += SLIM_THREADS) {
      const double v = j == i ? 0.0 : p.S[slim_cell(p.symmetric, n, i, j)];
      neg |= v < 0.0;
      w[j] = v;
    }
    const int any_neg = __syncthreads_or(neg);
    int* out_idx = p.out_idx + (size_t)i * p.topk;
    float* out_val = p.out_val + (size_t)i * p.topk;
    select_topk_nonzero(w, n, p.topk, any_neg, out_idx, out_val, p.out_cnt + i, wv, wi, &s_stop);
    __syncthreads();      // (s_stop, wv / wi and the row are reused by the next item)
  }
}

}  // namespace ganmf
