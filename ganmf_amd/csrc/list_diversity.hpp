// Intra-list diversity of the ranked lists (ganmf_evaluate_diversity; Base/Evaluation/metrics.py:405-452, Diversity_similarity):
// for one list l of length L the reference adds D[l_i, l_j] over i = 0 .. L-2 (the LAST item's row is never visited) and every
// j != i, and divides by L (L - 1); D is any [W, W] matrix with entries in [0, 1], not necessarily symmetric.
//
// One 256-thread workgroup per evaluated row.  The row's top-K list (mask_topk_kernel / cand_topk_kernel output, -1 padded at the
// end) is staged in LDS; len = its valid ids, L_c = min(c, len) per cut-off.  Wave w takes the list rows i = w, w + 4, ...; its lanes
// walk j = lane, lane + 64, ...: j is the fast index, so one wave gathers from ONE row of D at a time (D[l_i, :] through the
// list's columns -- element-granular, uncoalesced by nature; a row of D is read by every list that holds the item and stays in
// L2).  The ordered pair (i, j) belongs to the list cut at c iff max(i + 2, j + 1) <= L_c; it is added, in float64, to the bin of the
// SMALLEST cut-off that contains it (a per-thread LDS accumulator per ascending cut-off: no dynamic register indexing), and the
// prefix over the ascending cut-offs is taken once at the end -- the scheme eval_topk_body uses for its counts -- instead of one
// accumulator per (pair, cut-off).  Reduction in a fixed order: per-thread sums in walk order, wave butterfly, the four wave sums
// in index order.  No floating-point atomics: the same bytes on every call and handle.
// The user's value at c is sum / (L_c (L_c - 1)), and 0 when L_c < 2 (the reference divides by zero there); such a user still
// counts in the mean.
//
// Work: sum over rows of len^2 gathers, O(n K^2).  At K <= 50 and n = 6040 (ML-1M) that is 15 M gathers, small beside the
// 6040 x 3706 x k scoring product in front of it; at K = 1024 it is a million gathers per row, 6 G per ML-1M block, and this
// kernel then costs far more than the ranking -- the evaluators keep such cut-offs off the full-width device route anyway.
#pragma once

namespace ganmf {

struct ListDivP {
  const int* items;            // [n, K] recommended ids, -1 padded (a suffix)
  int K;
  const float* D;              // [W, W] row-major
  int W;
  int ncut;
  int cutoffs[EVAL_MAX_CUTOFFS];
  int order[EVAL_MAX_CUTOFFS]; // cut-off indices by ascending cut-off (ties: lower index first)
  double* out;                 // [n, ncut] per-user values, cut-offs in the caller's order
};
constexpr int LIST_DIV_MAX_K = 1024;   // GANMF_RECOMMEND_MAX_CUTOFF ints of LDS

__global__ __launch_bounds__(256) void list_diversity_kernel(const ListDivP p) {
  __shared__ int lst[LIST_DIV_MAX_K];
  __shared__ double acc[EVAL_MAX_CUTOFFS][256];
  __shared__ double wsum[4][EVAL_MAX_CUTOFFS];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < p.K; i += 256) lst[i] = p.items[(size_t)r * p.K + i];
  for (int b = 0; b < p.ncut; ++b) acc[b][tid] = 0.0;
  __syncthreads();
  int len = 0;                           // first padded position: the padding is a suffix
  {
    int hi = p.K;
    while (len < hi) {
      const int mid = (len + hi) >> 1;
      if (lst[mid] >= 0) len = mid + 1; else hi = mid;
    }
  }
  int asc[EVAL_MAX_CUTOFFS];             // the cut-offs ascending
#pragma unroll
  for (int b = 0; b < EVAL_MAX_CUTOFFS; ++b) asc[b] = b < p.ncut ? p.cutoffs[p.order[b]] : 0x7fffffff;
  for (int i = wave; i + 1 < len; i += 4) {          // rows 0 .. len-2
    const int li = lst[i];
    if ((unsigned)li >= (unsigned)p.W) continue;     // (never: the ranking writes ids of the score width)
    const float* __restrict__ drow = p.D + (size_t)li * p.W;
    for (int j = lane; j < len; j += 64) {
      if (j == i) continue;
      const int lj = lst[j];
      if ((unsigned)lj >= (unsigned)p.W) continue;
      const int m = max(i + 2, j + 1);               // the shortest cut list that holds the pair
      int b = 0;
#pragma unroll
      for (int q = 0; q < EVAL_MAX_CUTOFFS; ++q) b += asc[q] < m ? 1 : 0;
      if (b < p.ncut) acc[b][tid] += (double)drow[lj];
    }
  }
  for (int b = 0; b < p.ncut; ++b) {
    double s = acc[b][tid];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) wsum[wave][b] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int b = 0; b < p.ncut; ++b) {
      run += ((wsum[0][b] + wsum[1][b]) + wsum[2][b]) + wsum[3][b];
      const int ci = p.order[b];
      const int Lc = min(p.cutoffs[ci], len);
      p.out[(size_t)r * p.ncut + ci] = Lc < 2 ? 0.0 : run / ((double)Lc * (double)(Lc - 1));
    }
  }
}

// Sums over the n rows of the [n, ncol] per-user values, column blockIdx.y: 256 rows per workgroup through the LDS tree of
// eval_topk_body into partials[gridDim.x][ncol]; the host adds the block partials in block order (sum_block_partials).
__global__ __launch_bounds__(256) void column_block_sum_kernel(const double* __restrict__ vals, int n, int ncol, double* __restrict__ partials) {
  __shared__ double red[256];
  const int u = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y;
  red[threadIdx.x] = u < n ? vals[(size_t)u * ncol + col] : 0.0;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[(size_t)blockIdx.x * ncol + col] = red[0];
}

}  // namespace ganmf
