// p3_rows.hpp -- the graph-based item models P3alpha and RP3beta on the device: the three-step random walk of the reference's
// GraphBased/P3alphaRecommender.py:52-141 and RP3betaRecommender.py:49-151, W = top-k per column of (row-normalised) top-k per row of
// Piu^alpha . Pui^alpha (. diag(deg^-beta)).  The kernels of itemknn_rows.hpp are used as they are for the packing and the scores.
//
// Row pass: one workgroup per SOURCE item i, on the row builder of itemknn_fit_kernel (SimRowP, sim_row_accumulate: itemknn_rows.hpp;
// the slab is filled with row_scale[i] instead of the stored value).  Side 1 of the handle holds Pui^alpha by item (the
// pattern of the URM by item, the transition weights as values).  Piu^alpha has one value per item, row_scale[i] = (1 / deg_i)^alpha, at
// the users stored in column i: that is what the LDS slab of KNN_SLAB users holds (0 elsewhere).  Thread t owns the targets
// j = t, t + 256, ... and w_j = sum_u Piu[i, u] Pui[u, j] is one fp32 FMA chain fmaf(slab[u], val[q], acc) over ascending users; slabs
// are taken in ascending order, those without an entry of column i skipped.  Then one multiply by col_scale[j] (RP3beta's popularity
// penalty; absent for P3alpha), w_i = 0, and select_topk_nonzero (topk_rounds.hpp): topk arg-max rounds with ties to the smaller j; the
// non-zero picks are stored.
// itemknn_pack_kernel turns them into the compact row-major matrix R, columns ascending inside a row.
// Row normalisation: every row of R divided by the sum of the absolute values of its entries, summed in stored order in fp64.
// Column pass: one workgroup per TARGET item j holds column j of R as a dense vector over the source items (thread t owns the rows
// i = t, t + 256, ... and finds j in row i by binary search over its ascending columns), then runs the same select_topk_nonzero: col_topk
// largest, ties to the smaller i, zeros dropped.  It does no arithmetic: its values are bit copies.  Without a second selection
// (col_topk = 0) R is transposed instead: a histogram of its column ids, then an ordered compaction of every column (the same search,
// positions from a ballot over ascending i).  No floating-point atomic anywhere: two fits return the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include "itemknn_rows.hpp"

namespace ganmf {

struct P3RowP : SimRowP {      // side 1 holds Pui^alpha
  const float* row_scale;      // [n_items] (1 / deg_i)^alpha
  const float* col_scale;      // [n_items] deg_j^-beta, or null
};

struct P3ColP {
  const long long* r_indptr;   // R: source item x target item, targets ascending inside a row
  const int* r_idx;
  const float* r_val;
  int n_items;
  int topk;                    // <= min(KNN_MAX_TOPK, n_items)
  int row_lds;                 // 1: the dense column is the dynamic LDS; 0: row_glob + blockIdx.x * ld_row
  float* row_glob;
  long long ld_row;
  int* out_idx;                // [n_items, topk]
  float* out_val;
  int* out_cnt;
};

__global__ __launch_bounds__(KNN_THREADS) void p3_rows_kernel(const P3RowP p) {
  extern __shared__ __attribute__((aligned(16))) float p3_lds[];
  __shared__ float wv[4];
  __shared__ int wi[4];
  __shared__ int s_stop;
  const int tid = threadIdx.x;
  float* xs = p3_lds;
  float* w = p.row_lds ? p3_lds + p.slab : p.row_glob + (size_t)blockIdx.x * p.ld_row;
  const int n = p.n_items;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    // ---- w_j = sum_u Piu[i, u] Pui[u, j]: the slab holds the one value of row i of Piu ----
    const float rs = p.row_scale[i];
    sim_row_accumulate(p, xs, w, i, [rs](long long) { return rs; });
    // ---- the popularity penalty, w_i = 0 (thread t owns the same j as above) ----
    int neg = 0;
    for (int j = tid; j < n; j += KNN_THREADS) {
      float v = w[j];
      if (j == i) v = 0.f;
      else if (p.col_scale && v != 0.f) v *= p.col_scale[j];
      neg |= v < 0.f;
      w[j] = v;
    }
    const int any_neg = __syncthreads_or(neg);
    select_topk_nonzero(w, n, p.topk, any_neg, p.out_idx + (size_t)i * p.topk, p.out_val + (size_t)i * p.topk, p.out_cnt + i, wv, wi,
                        &s_stop);
    __syncthreads();      // (s_stop, wv / wi and the row are reused by the next item)
  }
}

// One 64-thread workgroup per row of R: the row divided by its L1 norm (sum in stored order, fp64; one rounding per value).
__global__ __launch_bounds__(64) void p3_normalize_kernel(const long long* __restrict__ indptr, float* __restrict__ val, int n) {
  __shared__ double s_sum;
  const int i = blockIdx.x;
  if (i >= n) return;
  const long long a = indptr[i], b = indptr[i + 1];
  if (a == b) return;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (long long q = a; q < b; ++q) s += fabs((double)val[q]);
    s_sum = s;
  }
  __syncthreads();
  const double s = s_sum;
  if (!(s > 0.0)) return;
  for (long long q = a + threadIdx.x; q < b; q += 64) val[q] = (float)((double)val[q] / s);
}

// value of R[i, j], 0 where nothing is stored
__device__ __forceinline__ bool p3_find(const long long* __restrict__ indptr, const int* __restrict__ idx, int i, int j, long long* at) {
  const long long a = indptr[i], b = indptr[i + 1];
  const long long q = knn_lower_bound(idx, a, b, j);
  *at = q;
  return q < b && idx[q] == j;
}

__global__ __launch_bounds__(KNN_THREADS) void p3_columns_kernel(const P3ColP p) {
  extern __shared__ __attribute__((aligned(16))) float p3_lds[];
  __shared__ float wv[4];
  __shared__ int wi[4];
  __shared__ int s_stop;
  const int tid = threadIdx.x;
  float* w = p.row_lds ? p3_lds : p.row_glob + (size_t)blockIdx.x * p.ld_row;
  const int n = p.n_items;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    int neg = 0;
    for (int i = tid; i < n; i += KNN_THREADS) {
      long long q;
      const float v = p3_find(p.r_indptr, p.r_idx, i, j, &q) ? p.r_val[q] : 0.f;
      neg |= v < 0.f;
      w[i] = v;
    }
    const int any_neg = __syncthreads_or(neg);
    select_topk_nonzero(w, n, p.topk, any_neg, p.out_idx + (size_t)j * p.topk, p.out_val + (size_t)j * p.topk, p.out_cnt + j, wv, wi,
                        &s_stop);
    __syncthreads();
  }
}

// col_topk = 0: the stored entries per column of R (integer atomics: the counts do not depend on the order) ...
__global__ __launch_bounds__(KNN_THREADS) void p3_count_kernel(const int* __restrict__ r_idx, long long nnz, int* __restrict__ cnt) {
  for (long long q = (long long)blockIdx.x * KNN_THREADS + threadIdx.x; q < nnz; q += (long long)gridDim.x * KNN_THREADS)
    atomicAdd(&cnt[r_idx[q]], 1);
}

// ... and column j of R to [out_indptr[j], out_indptr[j + 1]) with the source items ascending: 256 rows at a time, the place of a hit
// is the number of hits before it (ballot inside a wave, the waves in order)
__global__ __launch_bounds__(KNN_THREADS) void p3_transpose_kernel(const long long* __restrict__ r_indptr, const int* __restrict__ r_idx,
                                                                   const float* __restrict__ r_val, int n,
                                                                   const long long* __restrict__ out_indptr, int* __restrict__ out_idx,
                                                                   float* __restrict__ out_val) {
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    long long base = out_indptr[j];
    const long long last = out_indptr[j + 1];
    for (int i0 = 0; i0 < n && base < last; i0 += KNN_THREADS) {      // (base and last are the same in every thread)
      const int i = i0 + tid;
      long long q = 0;
      const bool hit = i < n && p3_find(r_indptr, r_idx, i, j, &q);
      const unsigned long long m = __ballot(hit);
      if (lane == 0) wcnt[wave] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
      for (int v = 0; v < 4; ++v) {
        if (v < wave) before += wcnt[v];
        total += wcnt[v];
      }
      if (hit) {
        const long long pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < last) { out_idx[pos] = i; out_val[pos] = r_val[q]; }
      }
      base += total;
      __syncthreads();
    }
  }
}

}  // namespace ganmf
