// itemknn_rows.hpp -- item-based nearest neighbours on the device: the similarity fit of the reference's Compute_Similarity_Python
// (Base/Similarity/Compute_Similarity_Python.py:209-384) and the sparse scoring product URM[users] . W_sparse
// (Base/BaseSimilarityMatrixRecommender.py:73-92).
//
// Fit: one workgroup per target item i.  The [n_items, n_items] matrix of dot products never exists: a workgroup holds ONE row of it
// -- w_j = sum_u x_ui x_uj for every j -- in LDS (KNN_ROW_LDS floats; wider catalogues: a private row in global memory, one per
// workgroup of the grid), applies the similarity's denominator, and selects the top-k of the row with select_topk_nonzero
// (topk_rounds.hpp, the arg-max rounds of mask_topk_kernel): ties go to the smaller item id, zeros are dropped.  The row builder,
// SimRowP and sim_row_accumulate, is shared with p3_rows_kernel (p3_rows.hpp); only what fills the slab differs.
//   w_j: column i of the URM (row i of side 1 of ganmf_als_set_confidence, users ascending) is expanded into a dense vector over one
//   slab of KNN_SLAB users in LDS; thread t owns the items j = t, t + 256, ... and walks column j's entries inside the slab in stored
//   order.  Slabs are taken in ascending order and slabs without an entry of column i are skipped, so every w_j is one fp32 FMA chain
//   over ascending users: no atomics, the same bytes on every call.
// Pack: the selected (neighbour, value) pairs of a column, sorted by ascending neighbour id (a bitonic network in LDS), go to their
// place in the compact matrix -- the order scipy gives a saved and re-loaded W_sparse, so both score bit for bit alike.
// Scores: a workgroup holds the dense profiles of G users in LDS (G x n_items floats) and thread t owns target items: every stored
// weight W[j, i] is read once per group of G users and multiplied into G accumulators; fp32 FMA chains in stored order, zeros where
// nothing is stored.  Catalogues above KNN_SCORE_LDS floats read the dense profiles from global memory instead.
#pragma once
#include <hip/hip_runtime.h>
#include "topk_rounds.hpp"

namespace ganmf {

constexpr int KNN_THREADS = 256;
static_assert(KNN_THREADS == TOPK_THREADS, "the fits select with the rounds of topk_rounds.hpp");
constexpr int KNN_MAX_TOPK = 1024;      // GANMF_ITEMKNN_MAX_TOPK: the selection's bound (GANMF_RECOMMEND_MAX_CUTOFF)
constexpr int KNN_SLAB = 8192;          // users per LDS slab of the fit (32 KiB)
constexpr int KNN_ROW_LDS = 28672;      // floats of the similarity row kept in LDS (112 KiB; with the slab 144 KiB of the CU's 160)
constexpr int KNN_SCORE_LDS = 32768;    // floats of dense profiles a scoring workgroup keeps in LDS (128 KiB)
constexpr int KNN_SCORE_GROUP = 16384;  // ... and what G > 1 users may take together (64 KiB: two workgroups per CU)
enum KnnKind : int { KNN_PRODUCT = 0, KNN_TANIMOTO = 1, KNN_DICE = 2, KNN_TVERSKY = 3, KNN_SHRINK_ONLY = 4, KNN_RAW = 5, KNN_KINDS = 6 };

// What the row builders of the item-similarity fits share (itemknn_fit_kernel here, p3_rows_kernel in p3_rows.hpp)
struct SimRowP {
  const long long* c_indptr;   // side 1: items x users, users ascending inside an item
  const int* c_users;
  const float* c_val;
  int n_items, n_users;
  int topk;                    // <= min(KNN_MAX_TOPK, n_items)
  int slab;                    // users per slab (<= KNN_SLAB): the first `slab` floats of the dynamic LDS
  int row_lds;                 // 1: the row follows the slab in LDS; 0: row_glob + blockIdx.x * ld_row
  float* row_glob;
  long long ld_row;
  int* out_idx;                // [n_items, topk] picks in descending order of value
  float* out_val;
  int* out_cnt;                // [n_items] stored picks (the non-zero ones)
};

struct KnnFitP : SimRowP {
  int kind;                    // KnnKind
  float s, shrink, p0, p1;     // s = shrink + 1e-6 (formed in float64 by the host)
  const float* den_a;          // [n_items], per kind (KnnKind); den_b: PRODUCT only
  const float* den_b;
};

// first position in [a, b) whose user is >= u
__device__ __forceinline__ long long knn_lower_bound(const int* __restrict__ users, long long a, long long b, int u) {
  while (a < b) {
    const long long m = (a + b) >> 1;
    if (users[m] < u) a = m + 1; else b = m;
  }
  return a;
}

// The slab walk: w_j = sum_u fill(q_u) c_val[u, j] for every j, where column i of side 1 -- expanded into the slab xs with fill(q) at
// the user of its stored entry q, 0 elsewhere -- is one factor and column j the other.  One slab of users at a time, ascending, slabs
// without an entry of column i skipped; thread t owns the items j = t, t + 256, ... so every w_j is one fp32 FMA chain over ascending
// users.  Called by the whole workgroup; ends behind a barrier.
template <typename FillFn>
__device__ __forceinline__ void sim_row_accumulate(const SimRowP& p, float* xs, float* w, int i, FillFn fill) {
  const int tid = threadIdx.x, n = p.n_items;
  const long long cs = p.c_indptr[i], ce = p.c_indptr[i + 1];
  for (int j = tid; j < n; j += KNN_THREADS) w[j] = 0.f;
  long long at = cs;      // first entry of column i not yet expanded (the same value in every thread)
  while (at < ce) {
    const int base = (p.c_users[at] / p.slab) * p.slab;      // the next slab that holds an entry of column i
    const long long top = (long long)base + p.slab;
    const long long end = top > p.n_users ? ce : knn_lower_bound(p.c_users, at, ce, (int)top);
    __syncthreads();      // the readers of the slab before this one (and the zero fill of w) are done
    for (int t = tid; t < p.slab; t += KNN_THREADS) xs[t] = 0.f;
    __syncthreads();
    for (long long q = at + tid; q < end; q += KNN_THREADS) xs[p.c_users[q] - base] = fill(q);
    __syncthreads();
    for (int j = tid; j < n; j += KNN_THREADS) {
      const long long a = p.c_indptr[j], b = p.c_indptr[j + 1];
      long long q = base == 0 ? a : knn_lower_bound(p.c_users, a, b, base);
      float acc = w[j];
      for (; q < b; ++q) {
        const int u = p.c_users[q];
        if (u >= top) break;
        acc = fmaf(xs[u - base], p.c_val[q], acc);
      }
      w[j] = acc;
    }
    at = end;
  }
  __syncthreads();
}

__device__ __forceinline__ float knn_value(const KnnFitP& p, float w, float dai, int j) {
  switch (p.kind) {
    case KNN_PRODUCT: return w / (dai * p.den_b[j] + p.s);
    case KNN_TANIMOTO: return w / (dai + p.den_a[j] - w + p.s);
    case KNN_DICE: return w / (dai + p.den_a[j] + p.s);
    case KNN_TVERSKY: return w / (w + (dai - w) * p.p0 + (p.den_a[j] - w) * p.p1 + p.s);
    case KNN_SHRINK_ONLY: return w / p.shrink;
    default: return w;
  }
}

__global__ __launch_bounds__(KNN_THREADS) void itemknn_fit_kernel(const KnnFitP p) {
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  __shared__ float wv[4];
  __shared__ int wi[4];
  __shared__ int s_stop;
  const int tid = threadIdx.x;
  float* xs = knn_lds;
  float* w = p.row_lds ? knn_lds + p.slab : p.row_glob + (size_t)blockIdx.x * p.ld_row;
  const int n = p.n_items;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    // ---- w_j = sum_u x_ui x_uj: the slab holds the stored values of column i ----
    sim_row_accumulate(p, xs, w, i, [&p](long long q) { return p.c_val[q]; });
    // ---- w_i = 0, the similarity's denominator (thread t owns the same j as above) ----
    const float dai = p.den_a ? p.den_a[i] : 0.f;
    int neg = 0;
    for (int j = tid; j < n; j += KNN_THREADS) {
      float v = w[j];
      if (j == i) v = 0.f;
      else if (v != 0.f) v = knn_value(p, v, dai, j);
      neg |= v < 0.f;
      w[j] = v;
    }
    const int any_neg = __syncthreads_or(neg);
    // ---- the topk largest of the row, the non-zero ones stored (Compute_Similarity_Python.py:346-356) ----
    select_topk_nonzero(w, n, p.topk, any_neg, p.out_idx + (size_t)i * p.topk, p.out_val + (size_t)i * p.topk, p.out_cnt + i, wv, wi,
                        &s_stop);
    __syncthreads();      // (s_stop, wv / wi and the row are reused by the next item)
  }
}

// One workgroup per item: its cnt[i] <= KNN_MAX_TOPK picks, sorted by ascending neighbour id, to indptr[i] of the compact matrix.
__global__ __launch_bounds__(KNN_THREADS) void itemknn_pack_kernel(const int* __restrict__ in_idx, const float* __restrict__ in_val,
                                                                   const int* __restrict__ cnt, int topk,
                                                                   const long long* __restrict__ indptr, int* __restrict__ out_idx,
                                                                   float* __restrict__ out_val) {
  __shared__ int si[KNN_MAX_TOPK];
  __shared__ float sv[KNN_MAX_TOPK];
  const int i = blockIdx.x, tid = threadIdx.x, c = cnt[i];
  if (c == 0) return;
  int m = 2;
  while (m < c) m <<= 1;      // (c <= KNN_MAX_TOPK, a power of two)
  for (int t = tid; t < m; t += KNN_THREADS) {
    si[t] = t < c ? in_idx[(size_t)i * topk + t] : 0x7fffffff;
    sv[t] = t < c ? in_val[(size_t)i * topk + t] : 0.f;
  }
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < m; t += KNN_THREADS) {
        const int x = t ^ j;
        if (x > t) {
          const bool up = (t & k) == 0;
          const int a = si[t], b = si[x];
          if ((a > b) == up) {
            si[t] = b; si[x] = a;
            const float f = sv[t];
            sv[t] = sv[x]; sv[x] = f;
          }
        }
      }
      __syncthreads();
    }
  const long long o = indptr[i];
  for (int t = tid; t < c; t += KNN_THREADS) { out_idx[o + t] = si[t]; out_val[o + t] = sv[t]; }
}

struct KnnScoreP {
  const long long* r_indptr;   // side 0: users x items (the weighted URM), items ascending without repeats inside a user
  const int* r_items;
  const float* r_val;
  const long long* w_indptr;   // W by target item
  const int* w_nbr;
  const float* w_val;
  const int* ids;              // [n] scored users
  int n, n_items;
  float* out;                  // [n, ldo]
  int ldo;
  float* dense;                // global route: [round_up(n, 8), ldd] dense profiles (zero-filled, then knn_densify_kernel)
  long long ldd;
};

// global route: the profile of scored row r into its (zeroed) dense row
__global__ __launch_bounds__(KNN_THREADS) void itemknn_densify_kernel(const KnnScoreP p) {
  const int r = blockIdx.x, u = p.ids[r];
  float* d = p.dense + (size_t)r * p.ldd;
  for (long long q = p.r_indptr[u] + threadIdx.x; q < p.r_indptr[u + 1]; q += KNN_THREADS) d[p.r_items[q]] = p.r_val[q];
}

// grid (ceil(n / G), item chunks): workgroup (g, c) scores the users [g G, g G + G) for the items c * 256 + t, stepping by 256 chunks
template <int G, bool kLds>
__global__ __launch_bounds__(KNN_THREADS) void itemknn_score_kernel(const KnnScoreP p) {
  extern __shared__ __attribute__((aligned(16))) float knn_prof[];
  const int tid = threadIdx.x, r0 = blockIdx.x * G, n = p.n_items;
  const float* prof;
  size_t stride;
  if (kLds) {
    for (int t = tid; t < G * n; t += KNN_THREADS) knn_prof[t] = 0.f;
    __syncthreads();
    for (int g = 0; g < G; ++g) {
      if (r0 + g >= p.n) break;
      const int u = p.ids[r0 + g];
      for (long long q = p.r_indptr[u] + tid; q < p.r_indptr[u + 1]; q += KNN_THREADS) knn_prof[g * n + p.r_items[q]] = p.r_val[q];
    }
    __syncthreads();
    prof = knn_prof; stride = (size_t)n;
  } else {
    prof = p.dense + (size_t)r0 * p.ldd; stride = (size_t)p.ldd;      // (rows past n exist and are zero)
  }
  for (int i = blockIdx.y * KNN_THREADS + tid; i < n; i += gridDim.y * KNN_THREADS) {
    float acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.f;
    const long long b = p.w_indptr[i + 1];
    for (long long q = p.w_indptr[i]; q < b; ++q) {
      const int j = p.w_nbr[q];
      const float wv = p.w_val[q];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = fmaf(prof[g * stride + j], wv, acc[g]);
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (r0 + g < p.n) p.out[(size_t)(r0 + g) * p.ldo + i] = acc[g];
  }
}

}  // namespace ganmf
