// nmf_rows.hpp -- the kernels of ganmf_nmf_mu / ganmf_nmf_cd / ganmf_nmf_error (lib/abi_nmf.inc): the two solvers of
// sklearn.decomposition.NMF as the reference's MatrixFactorization/NMFRecommender.py:65-78 runs them (all regularisation 0).  The
// sparse products X H^T and X^T W are svd_spmm_kernel's, the Gram matrices H H^T and W^T W the library's fp32 MFMA GEMM; what is here
// is everything else.  Both factors are stored by rows with k columns: W [n_users, ld] and H^T [n_items, ld], so that either half of an
// iteration is the same routine on (side, row factor, column factor).
//
// nmf_mu_kernel        the multiplicative update behind its denominator: F[i, c] *= num[i, c] / den with a denominator of exactly 0
//   replaced, den = (F . G)[i, c] as the library's fp32 GEMM left it (G the k x k Gram matrix of the OTHER factor), or a broadcast
//   vector (Kullback-Leibler).  One element-wise pass.  A row kernel that kept den out of memory (the row panel in LDS, G from L2)
//   was measured beside it and was slower: 28.3 against 11.5 us per half at k = 100 (GEMM included), 10.8 against 10.1 at k = 25.
// nmf_cd_rows_kernel   one wave per row: the row of F and its gradient g = F[i, :] G - B[i, :] (B = X . other factor) live in
//   registers (column c in lane c % 64, register c / 64), the permutation in LDS, G in L2.  For every coordinate t in permutation
//   order: grad = g[t], the projected gradient joins the row's violation (float64), F[i, t] = max(F[i, t] - grad / G[t, t], 0) when
//   G[t, t] != 0, and g += delta G[t, :].  The incremental form: no reduction per step.  sklearn's form (one dot product and one
//   butterfly sum per coordinate) differs only in rounding and was measured slower: 74.3 against 64.0 us per half at k = 100, 19.7
//   against 15.2 at k = 25.
// nmf_sampled_kernel   q_e = x_e / max(a_r . b_c, EPS) for every stored entry of one CSR orientation, written to a value array that
//   svd_spmm_kernel then reads through its `val` pointer.  The work is split by stored entries, not by rows: a wave takes 256
//   consecutive CSR positions (their rows come from an index array, nmf_rowidx_kernel), 4, 8 or 16 lanes per entry by k (one float4
//   of both rows each, then shuffles), four entries of a lane group in flight.  With `err` it also leaves the chunk's two sums of the
//   Kullback-Leibler divergence, sum x log(x / max(wh, EPS)) and sum x over x > EPS, in float64 -- the error is the same single
//   pass over the stored entries.
// nmf_colsum_kernel    column sums of a factor in float64, rounded once to float32.
// nmf_dot_kernel / nmf_sum_kernel   sum_ij A_ij B_ij in float64 as 256 partial sums and their total: the traces of the Frobenius error,
//   |X|^2, and the totals of per-row values (violations, divergence sums).
// Everything sums in a fixed order and nothing uses a floating-point atomic: two calls on the same state return the same bytes.
#pragma once
#include <hip/hip_runtime.h>

namespace ganmf {

constexpr int NMF_MAX_FACTORS = 270;      // GANMF_NMF_MAX_FACTORS: what init = "nndsvda" admits (GANMF_SVD_MAX_RANDOM - 10)
constexpr int NMF_NT = (NMF_MAX_FACTORS + 63) / 64;      // registers per row and lane of nmf_cd_rows_kernel
constexpr float NMF_EPS = 1.1920929e-7f;                 // np.finfo(np.float32).eps
constexpr float NMF_H_FLOOR = 2.220446049250313e-16f;    // np.finfo(np.float64).eps: smaller entries of H become 0 (Kullback-Leibler)
constexpr int NMF_THREADS = 256;
constexpr int NMF_SAMP_FLIGHT = 4;        // entries of one slot of nmf_sampled_kernel in flight
constexpr int NMF_SAMP_CHUNK = 256;       // CSR positions per wave of nmf_sampled_kernel
constexpr int NMF_PARTS = 256;            // partial sums of nmf_dot_kernel
constexpr int NMF_SUM_THREADS = 1024;

// column t of a row kept as (lane c % 64, register c / 64), on every lane
template <int NT>
__device__ inline float nmf_bcast(const float (&a)[NT], int t) {
  float v = 0.f;
#pragma unroll
  for (int u = 0; u < NT; ++u)
    if ((t >> 6) == u) v = a[u];
  return __shfl(v, t & 63);
}

struct NmfCdP {
  float* F;                  // [rows, ldf]
  const float* B;            // [rows, ldb]: X . (other factor)
  const float* G;            // [k, ldg]
  const int* perm;           // [k], every value in [0, k)
  double* viol;              // [rows]: the row's sum of |projected gradient|
  int ldf, ldb, ldg, rows, k;
};

template <int NT>
__global__ __launch_bounds__(NMF_THREADS) void nmf_cd_rows_kernel(NmfCdP p) {
  __shared__ int perm_s[NMF_NT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = p.k;
  for (int i = tid; i < k; i += NMF_THREADS) perm_s[i] = p.perm[i];
  __syncthreads();
  const long long row = (long long)blockIdx.x * (NMF_THREADS / 64) + wave;
  if (row >= p.rows) return;
  float w[NT], b[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int c = lane + 64 * u;
    w[u] = c < k ? p.F[(size_t)row * p.ldf + c] : 0.f;
    b[u] = c < k ? p.B[(size_t)row * p.ldb + c] : 0.f;
  }
  double viol = 0.0;
  // g = F[i, :] G - B[i, :] once, then g += delta G[t, :] behind every change: no reduction per step
  float gr[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) gr[u] = -b[u];
  for (int t = 0; t < k; ++t) {
    const float wt = nmf_bcast<NT>(w, t);
    if (wt == 0.f) continue;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int c = lane + 64 * u;
      gr[u] += wt * (c < k ? p.G[(size_t)t * p.ldg + c] : 0.f);
    }
  }
  for (int s = 0; s < k; ++s) {
    const int t = perm_s[s];
    float g[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int c = lane + 64 * u;
      g[u] = c < k ? p.G[(size_t)t * p.ldg + c] : 0.f;
    }
    const float grad = nmf_bcast<NT>(gr, t), wt = nmf_bcast<NT>(w, t), hess = nmf_bcast<NT>(g, t);
    const float pg = wt == 0.f ? fminf(0.f, grad) : grad;
    viol += (double)fabsf(pg);
    if (hess != 0.f) {
      const float nw = fmaxf(wt - grad / hess, 0.f), delta = nw - wt;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        if (lane + 64 * u == t) w[u] = nw;
        gr[u] += delta * g[u];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int c = lane + 64 * u;
    if (c < k) p.F[(size_t)row * p.ldf + c] = w[u];
  }
  if (lane == 0) p.viol[row] = viol;
}

struct NmfMuP {
  float* F;                  // [rows, ldf]: the factor that is updated
  const float* num;          // [rows, ldn]
  const float* den;          // [rows, ldd]: F . G as the GEMM left it, or with ldd == 0 the broadcast vector [k]
  int ldf, ldn, ldd, rows, k;
  float zero_den;            // what a denominator of exactly 0 becomes
  int floor_h;               // results below NMF_H_FLOOR become 0
};

__global__ __launch_bounds__(NMF_THREADS) void nmf_mu_kernel(NmfMuP p) {
  const long long total = (long long)p.rows * p.k;
  for (long long i = (long long)blockIdx.x * NMF_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * NMF_THREADS) {
    const long long r = i / p.k;
    const int c = (int)(i - r * p.k);
    float d = p.den[(size_t)r * p.ldd + c];
    if (d == 0.f) d = p.zero_den;
    float v = p.F[(size_t)r * p.ldf + c] * (p.num[(size_t)r * p.ldn + c] / d);
    if (p.floor_h && v < NMF_H_FLOOR) v = 0.f;
    p.F[(size_t)r * p.ldf + c] = v;
  }
}

// rowidx[e] = the row of CSR position e: one wave per row
__global__ __launch_bounds__(NMF_THREADS) void nmf_rowidx_kernel(const long long* indptr, int n_rows, int* rowidx) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (NMF_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  for (long long e = indptr[r] + lane; e < indptr[r + 1]; e += 64) rowidx[e] = (int)r;
}

struct NmfSampP {
  const int* rowidx;         // [nnz] row of every CSR position (nmf_rowidx_kernel)
  const int* indices;
  const float* x;            // the stored values
  const float* A;            // [n_rows, lda]: the factor of the CSR's rows, pad columns zero
  const float* Bm;           // [n_cols, ldb]: the factor of its columns, pad columns zero
  float* q;                  // [nnz] x / max(a . b, EPS), or null
  double* err;               // [chunks, 2] (sum x log(x / max(a . b, EPS)), sum x) over x > EPS of a chunk's entries, or null
  long long nnz;
  int lda, ldb, nc4, lanes;  // nc4 = ceil(k / 4); lanes per entry: 4, 8 or 16
};

// A wave takes the NMF_SAMP_CHUNK consecutive CSR positions of its chunk, whatever rows they belong to: a row of thousands of entries
// is spread over many waves.  `lanes` lanes form a slot (one float4 of both factor rows each, then log2(lanes) shuffles: every lane of
// the slot ends with the same bits, and a pair (i, j) gives the same bits in either orientation); a slot takes the positions base +
// slot, base + slots + slot, ...: NMF_SAMP_FLIGHT of them per round, their factor rows in flight together.  The loop is uniform over
// the wave: the shuffles are reached by all 64 lanes.
__global__ __launch_bounds__(NMF_THREADS) void nmf_sampled_kernel(NmfSampP p) {
  const int tid = threadIdx.x, lane = tid & 63, lanes = p.lanes, slots = 64 / lanes, sub = lane / lanes, l = lane - sub * lanes;
  const long long chunk = (long long)blockIdx.x * (NMF_THREADS / 64) + (tid >> 6);
  const long long beg = chunk * NMF_SAMP_CHUNK;
  if (beg >= p.nnz) return;
  const long long end = beg + NMF_SAMP_CHUNK < p.nnz ? beg + NMF_SAMP_CHUNK : p.nnz;
  double e_log = 0.0, e_sum = 0.0;
  for (long long base = beg; base < end; base += slots * NMF_SAMP_FLIGHT) {
    const float4* a4[NMF_SAMP_FLIGHT];
    const float4* b4[NMF_SAMP_FLIGHT];
    float s[NMF_SAMP_FLIGHT];
#pragma unroll
    for (int u = 0; u < NMF_SAMP_FLIGHT; ++u) {
      const long long e = base + slots * u + sub;
      const bool live = e < end;      // (a dead slot reads row 0 of both factors: valid memory, its result is dropped)
      a4[u] = reinterpret_cast<const float4*>(p.A + (live ? (size_t)p.rowidx[e] * p.lda : 0));
      b4[u] = reinterpret_cast<const float4*>(p.Bm + (live ? (size_t)p.indices[e] * p.ldb : 0));
      s[u] = 0.f;
    }
    for (int c = l; c < p.nc4; c += lanes) {
#pragma unroll
      for (int u = 0; u < NMF_SAMP_FLIGHT; ++u) {
        const float4 a = a4[u][c], b = b4[u][c];
        s[u] += a.x * b.x; s[u] += a.y * b.y; s[u] += a.z * b.z; s[u] += a.w * b.w;
      }
    }
#pragma unroll
    for (int u = 0; u < NMF_SAMP_FLIGHT; ++u) {
      const long long e = base + slots * u + sub;
      float t = s[u];
      for (int o = lanes >> 1; o >= 1; o >>= 1) t += __shfl_xor(t, o);
      if (e < end && l == 0) {
        const float x = p.x[e], wh = fmaxf(t, NMF_EPS);
        if (p.q) p.q[e] = x / wh;
        if (p.err && x > NMF_EPS) {
          e_log += (double)x * log((double)x / (double)wh);
          e_sum += (double)x;
        }
      }
    }
  }
  if (p.err) {      // the slots in slot order
    double tl = 0.0, ts = 0.0;
    for (int sl = 0; sl < slots; ++sl) {
      tl += __shfl(e_log, sl * lanes);
      ts += __shfl(e_sum, sl * lanes);
    }
    if (lane == 0) {
      p.err[2 * chunk] = tl;
      p.err[2 * chunk + 1] = ts;
    }
  }
}

// out[c] = sum_r A[r, c], c < k: 64 columns per workgroup, 16 row lanes of stride 16, float64
__global__ __launch_bounds__(NMF_SUM_THREADS) void nmf_colsum_kernel(const float* A, int lda, int rows, int k, float* out) {
  __shared__ double red[NMF_SUM_THREADS];
  const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6, c = blockIdx.x * 64 + cl;
  double s = 0.0;
  if (c < k)
    for (int r = rl; r < rows; r += NMF_SUM_THREADS / 64) s += (double)A[(size_t)r * lda + c];
  red[tid] = s;
  __syncthreads();
  for (int o = NMF_SUM_THREADS / 128; o >= 1; o >>= 1) {
    if (rl < o) red[tid] += red[tid + 64 * o];
    __syncthreads();
  }
  if (rl == 0 && c < k) out[c] = (float)red[cl];
}

// part[block] = sum over the block's rows (block, block + NMF_PARTS, ...) of sum_c A[r, c] B[r, c]; an element whose flat index
// r * cols + c reaches `total` is left out (a vector laid out as rows of `cols`)
__global__ __launch_bounds__(NMF_THREADS) void nmf_dot_kernel(const float* A, int lda, const float* Bm, int ldb, int rows, int cols,
                                                              long long total, double* part) {
  __shared__ double red[NMF_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int r = blockIdx.x; r < rows; r += NMF_PARTS)
    for (int c = tid; c < cols; c += NMF_THREADS)
      if ((long long)r * cols + c < total) s += (double)A[(size_t)r * lda + c] * (double)Bm[(size_t)r * ldb + c];
  red[tid] = s;
  __syncthreads();
  for (int o = NMF_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

// out[0] = (add ? out[0] : 0) + sum_i in[i * stride], i < n: one workgroup, a fixed tree
__global__ __launch_bounds__(NMF_SUM_THREADS) void nmf_sum_kernel(const double* in, long long n, int stride, double* out, int add) {
  __shared__ double red[NMF_SUM_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long i = tid; i < n; i += NMF_SUM_THREADS) s += in[i * stride];
  red[tid] = s;
  __syncthreads();
  for (int o = NMF_SUM_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[0] = (add ? out[0] : 0.0) + red[0];
}

}  // namespace ganmf
