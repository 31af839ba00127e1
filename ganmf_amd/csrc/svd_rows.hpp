// svd_rows.hpp -- the kernels of ganmf_pure_svd (lib/abi_svd.inc): a randomized truncated SVD of the handle's weighted sparse matrix
// (sklearn.utils.extmath.randomized_svd as the reference's MatrixFactorization/PureSVDRecommender.py:29-37 calls it).  The dense
// products Y^T Y, Y L^-T, Q W run on the library's fp32 MFMA GEMM; what is here is everything else:
//
// svd_spmm_kernel      Y[r, :] = sum_j a_rj Q[c_j, :] for one CSR side and a dense panel [cols, l] with a padded leading dimension.
//   A row of the panel is read by a GROUP of nc4 = ceil(l / 4) threads, one float4 each (one contiguous 4 l-byte segment per stored
//   entry); a row of the matrix is shared by `gpr` groups (group g takes the entries g, g + gpr, ...: four loads in flight each), a
//   workgroup of 256 threads holds 256 / nc4 groups: rows_per_wg rows of gpr = 4 groups while l <= 128, else one row over all of its
//   groups.  The groups' partial sums meet in LDS and are added in group order: a fixed order, no atomics.  A row without an
//   entry writes zeros.  Bound by the gather: every stored entry moves 4 l bytes out of a panel that L2 (or the MALL) holds.
// svd_chol_inv_kernel  one workgroup of 1024 threads: G = L L^T on the packed lower triangle in LDS (right-looking, one column per
//   step: l (l + 1) / 2 floats, 157 360 B of dynamic LDS at l = 280), then L^-1 in place row by row (four lanes per column), written
//   out as a dense lower-triangular [l, ldx] matrix with zeros above the diagonal.  A pivot that is not positive and finite is replaced by 1 (so that nothing
//   downstream faults on it) and reported through flag[0] / flag[1] with plain stores.
// svd_jacobi_kernel    one workgroup: one-sided (Hestenes) Jacobi on the l x l Gram matrix, kept in global memory (L2-resident:
//   313 KB at l = 280 does not fit LDS).  Row j of the buffer is column j of A = G (G is symmetric); a sweep is the n - 1 rounds of a
//   round-robin tournament, a round's n / 2 disjoint pairs go round the 16 waves, one barrier per round.  A pair's two columns live
//   in registers: three dot products by a shuffle butterfly (every lane ends with the same bits), rotation, store.  A pair rotates
//   while |a_p . a_q| > tol / 4 |a_p| |a_q| and COUNTS as not converged while it is > tol |a_p| |a_q|, tol = sqrt(l) 2^-23 (LAPACK's
//   sgesvj); the solver stops after the first sweep that counted nothing, or reports SVD_EIG_MAX_SWEEPS sweeps without that.
//   On exit column j is lambda_j w_j: lam[j] = its norm.
// svd_select_kernel    descending order of lam by rank counting (ties by index) and the [l, k] matrix the two final products multiply
//   with: W = columns / lambda.
// svd_finish_kernel    one workgroup per factor column: sigma_c = |(Z W)[:, c]|, the scales sigma and 1 / sigma of the transposed
//   case, and the sign rule: arg-max of |USER[:, c]| (first index on ties), both columns negated when that entry is negative
//   (sklearn's svd_flip as randomized_svd calls it).
// Everything sums in a fixed order: two calls on the same state return the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace ganmf {

constexpr int SVD_MAX_RANDOM = 280;      // GANMF_SVD_MAX_RANDOM: the packed triangle of svd_chol_inv_kernel has to fit 160 KiB of LDS
constexpr int SVD_SPMM_THREADS = 256;
constexpr int SVD_WG = 1024;             // the one-workgroup kernels
constexpr int SVD_EIG_MAX_SWEEPS = 30;
constexpr int SVD_EIG_NT = (SVD_MAX_RANDOM + 63) / 64;      // registers per column and lane
static_assert(SVD_MAX_RANDOM <= 2 * (SVD_WG / 4), "svd_chol_inv_kernel inverts in at most two passes of SVD_WG / 4 columns");

__device__ inline int svd_tri(int r) { return r * (r + 1) / 2; }

struct SvdSpmmP {
  const long long* indptr;   // CSR over n_rows
  const int* indices;
  const float* val;
  const float* Q;            // [cols, ldq], columns l .. ldq - 1 zero
  float* Y;                  // [n_rows, ldy]
  int ldq, ldy, n_rows;
  int nc4, gpr, rows_per_wg; // threads per group, groups per row, rows per workgroup: rows_per_wg * gpr * nc4 <= 256
};

__global__ __launch_bounds__(SVD_SPMM_THREADS) void svd_spmm_kernel(SvdSpmmP p) {
  __shared__ float4 part[SVD_SPMM_THREADS];
  const int tid = threadIdx.x;
  const int grp = tid / p.nc4, c4 = tid - grp * p.nc4;
  const int slot = grp / p.gpr, g = grp - slot * p.gpr;
  const long long r = (long long)blockIdx.x * p.rows_per_wg + slot;
  const bool live = slot < p.rows_per_wg && r < p.n_rows;
  if (live) {
    const long long end = p.indptr[r + 1];
    long long e = p.indptr[r] + g;
    const long long st = p.gpr;
    const float* q = p.Q + 4 * c4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; e + 3 * st < end; e += 4 * st) {      // four entries of this group in flight
      const int j0 = p.indices[e], j1 = p.indices[e + st], j2 = p.indices[e + 2 * st], j3 = p.indices[e + 3 * st];
      const float a0 = p.val[e], a1 = p.val[e + st], a2 = p.val[e + 2 * st], a3 = p.val[e + 3 * st];
      const float4 v0 = *reinterpret_cast<const float4*>(q + (size_t)j0 * p.ldq);
      const float4 v1 = *reinterpret_cast<const float4*>(q + (size_t)j1 * p.ldq);
      const float4 v2 = *reinterpret_cast<const float4*>(q + (size_t)j2 * p.ldq);
      const float4 v3 = *reinterpret_cast<const float4*>(q + (size_t)j3 * p.ldq);
      acc.x += a0 * v0.x; acc.y += a0 * v0.y; acc.z += a0 * v0.z; acc.w += a0 * v0.w;
      acc.x += a1 * v1.x; acc.y += a1 * v1.y; acc.z += a1 * v1.z; acc.w += a1 * v1.w;
      acc.x += a2 * v2.x; acc.y += a2 * v2.y; acc.z += a2 * v2.z; acc.w += a2 * v2.w;
      acc.x += a3 * v3.x; acc.y += a3 * v3.y; acc.z += a3 * v3.z; acc.w += a3 * v3.w;
    }
    for (; e < end; e += st) {
      const float a = p.val[e];
      const float4 v = *reinterpret_cast<const float4*>(q + (size_t)p.indices[e] * p.ldq);
      acc.x += a * v.x; acc.y += a * v.y; acc.z += a * v.z; acc.w += a * v.w;
    }
    part[tid] = acc;
  }
  __syncthreads();
  if (live && g == 0) {      // the groups of this row, in group order
    float4 s = part[tid];
    for (int o = 1; o < p.gpr; ++o) {
      const float4 v = part[tid + o * p.nc4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(p.Y + (size_t)r * p.ldy + 4 * c4) = s;
  }
}

struct SvdCholP {
  const float* G;            // [l, ldg], the lower triangle is read
  float* X;                  // L^-1 as a dense [l, ldx] matrix, zeros above the diagonal
  int ldg, ldx, l;
  int* flag;                 // flag[0]: code of the FIRST stage that failed in this call (0: none), flag[1]: its pivot (1-based)
  int code;
};

// dynamic LDS: the packed triangle and nothing else (157 360 B at l = 280; the failure word bad_s is 4 static bytes beside it)
inline size_t svd_chol_lds_bytes(int l) { return (size_t)l * (l + 1) / 2 * sizeof(float); }

__global__ __launch_bounds__(SVD_WG) void svd_chol_inv_kernel(SvdCholP p) {
  extern __shared__ float svd_Ls[];
  __shared__ int bad_s;
  float* const Ls = svd_Ls;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = SVD_WG / 64, l = p.l;
  for (int r = wave; r < l; r += nw)
    for (int c = lane; c <= r; c += 64) Ls[svd_tri(r) + c] = p.G[(size_t)r * p.ldg + c];
  if (tid == 0) bad_s = 0;
  __syncthreads();
  // ---- L L^T, one column per step ----
  for (int j = 0; j < l; ++j) {
    float d = Ls[svd_tri(j) + j];
    if (!(d > 0.f && d <= FLT_MAX)) {
      if (tid == 0 && bad_s == 0) bad_s = j + 1;
      d = 1.f;
    }
    const float s = sqrtf(d);
    for (int i = j + 1 + tid; i < l; i += SVD_WG) Ls[svd_tri(i) + j] /= s;
    __syncthreads();      // column j is final below the diagonal; every thread has read the pivot
    if (tid == 0) Ls[svd_tri(j) + j] = s;
    for (int r = j + 1 + wave; r < l; r += nw) {
      const float lr = Ls[svd_tri(r) + j];
      for (int c = j + 1 + lane; c <= r; c += 64) Ls[svd_tri(r) + c] -= lr * Ls[svd_tri(c) + j];
    }
    __syncthreads();
  }
  // ---- X = L^-1 in place, row by row: X[i][c] = -(sum_{t = c}^{i - 1} L[i][t] X[t][c]) / L[i][i], X[i][i] = 1 / L[i][i].  Column c is
  // owned by four neighbouring lanes (quarter q takes t = c + q, c + q + 4, ...; added by two shuffles: every lane of the four ends with
  // the same bits), 256 columns per pass ----
  const int q = tid & 3;
  for (int i = 0; i < l; ++i) {
    const float* li = Ls + svd_tri(i);
    const float dinv = 1.f / li[i];
    float xs[2] = {0.f, 0.f};
    for (int pass = 0; pass * (SVD_WG / 4) <= i; ++pass) {      // (uniform: the second pass only from row 256 on)
      const int c = (tid >> 2) + pass * (SVD_WG / 4);
      float s = 0.f;
      if (c < i)
        for (int t = c + q; t < i; t += 4) s += li[t] * Ls[svd_tri(t) + c];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      xs[pass] = c < i ? -s * dinv : dinv;
    }
    __syncthreads();      // row i of L has been read by everyone
    for (int pass = 0; pass * (SVD_WG / 4) <= i; ++pass) {
      const int c = (tid >> 2) + pass * (SVD_WG / 4);
      if (q == 0 && c <= i) Ls[svd_tri(i) + c] = xs[pass];
    }
    __syncthreads();
  }
  for (int r = wave; r < l; r += nw)
    for (int c = lane; c < l; c += 64) p.X[(size_t)r * p.ldx + c] = c <= r ? Ls[svd_tri(r) + c] : 0.f;
  if (tid == 0 && bad_s && p.flag[0] == 0) { p.flag[0] = p.code; p.flag[1] = bad_s; }
}

struct SvdEigP {
  float* A;                  // [l, lda]: the Gram matrix on entry (row j = column j), lambda_j w_j in row j on exit
  int lda, l;
  float tol;
  float* lam;                // [l]
  int* flag;                 // as SvdCholP::flag; flag[2]: sweeps run
  int code;
};

__device__ inline float svd_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(SVD_WG) void svd_jacobi_kernel(SvdEigP p) {
  __shared__ int cnt_s[SVD_WG / 64];
  __shared__ int done_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = SVD_WG / 64, l = p.l;
  const int n = (l + 1) & ~1, half = n / 2;      // an odd l plays with a bye
  int sweep = 0;
  bool done = l < 2;
  while (!done && sweep < SVD_EIG_MAX_SWEEPS) {
    int mycnt = 0;
    for (int s = 0; s < n - 1; ++s) {
      for (int j = wave; j < half; j += nw) {
        const int a = j == 0 ? n - 1 : (s + j) % (n - 1);
        const int b = j == 0 ? s : (s - j + n - 1) % (n - 1);
        if (a >= l || b >= l) continue;
        float* const ap = p.A + (size_t)(a < b ? a : b) * p.lda;
        float* const aq = p.A + (size_t)(a < b ? b : a) * p.lda;
        float x[SVD_EIG_NT], y[SVD_EIG_NT];
        float alpha = 0.f, beta = 0.f, gamma = 0.f;
#pragma unroll
        for (int t = 0; t < SVD_EIG_NT; ++t) {
          const int i = lane + 64 * t;
          x[t] = i < l ? ap[i] : 0.f;
          y[t] = i < l ? aq[i] : 0.f;
          alpha += x[t] * x[t];
          beta += y[t] * y[t];
          gamma += x[t] * y[t];
        }
        alpha = svd_wave_sum(alpha);
        beta = svd_wave_sum(beta);
        gamma = svd_wave_sum(gamma);
        const float lim = sqrtf(alpha) * sqrtf(beta);
        if (!(fabsf(gamma) > 0.25f * p.tol * lim)) continue;      // (also: a column of zeros, anything not finite)
        if (fabsf(gamma) > p.tol * lim) ++mycnt;
        const float zeta = (beta - alpha) / (2.f * gamma);
        const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
        const float c = 1.f / sqrtf(1.f + t * t), sn = c * t;
#pragma unroll
        for (int u = 0; u < SVD_EIG_NT; ++u) {
          const int i = lane + 64 * u;
          if (i < l) {
            ap[i] = c * x[u] - sn * y[u];
            aq[i] = sn * x[u] + c * y[u];
          }
        }
      }
      __syncthreads();      // the round's pairs are disjoint; the next round reads what this one stored
    }
    if (lane == 0) cnt_s[wave] = mycnt;
    __syncthreads();
    if (tid == 0) {
      int total = 0;
      for (int w = 0; w < nw; ++w) total += cnt_s[w];
      done_s = total == 0;
    }
    __syncthreads();
    done = done_s != 0;
    ++sweep;
  }
  for (int j = wave; j < l; j += nw) {
    const float* aj = p.A + (size_t)j * p.lda;
    float s = 0.f;
    for (int i = lane; i < l; i += 64) s += aj[i] * aj[i];
    s = svd_wave_sum(s);
    if (lane == 0) p.lam[j] = sqrtf(s);
  }
  if (tid == 0) {
    p.flag[2] = sweep;
    if (!done && p.flag[0] == 0) { p.flag[0] = p.code; p.flag[1] = sweep; }
  }
}

struct SvdSelP {
  const float* A;            // svd_jacobi_kernel's output
  const float* lam;
  int lda, l, k;
  float* W;                  // [l, ldw]: the first k eigenvectors in descending order of lambda, what both final products multiply with
  int ldw;
  int* flag;
  int code;
};

__global__ __launch_bounds__(SVD_WG) void svd_select_kernel(SvdSelP p) {
  __shared__ float lam_s[SVD_MAX_RANDOM];
  __shared__ int order[SVD_MAX_RANDOM];
  __shared__ int bad_s;
  const int tid = threadIdx.x, l = p.l, k = p.k;
  if (tid < l) { lam_s[tid] = p.lam[tid]; order[tid] = tid; }
  if (tid == 0) bad_s = 0;
  __syncthreads();
  int rank = 0;
  if (tid < l) {
    const float mine = lam_s[tid];
    for (int i = 0; i < l; ++i) rank += (lam_s[i] > mine || (lam_s[i] == mine && i < tid)) ? 1 : 0;
  }
  __syncthreads();
  if (tid < l) order[rank] = tid;      // (a permutation unless something is not a number; always inside [0, l))
  __syncthreads();
  if (tid < k) {
    const float lm = lam_s[order[tid]];
    if (!(lm > 0.f && lm <= FLT_MAX)) bad_s = tid + 1;      // (any of them: the flag is what matters)
  }
  __syncthreads();
  for (int idx = tid; idx < l * k; idx += SVD_WG) {
    const int i = idx / k, c = idx - i * k, j = order[c];
    p.W[(size_t)i * p.ldw + c] = p.A[(size_t)j * p.lda + i] / lam_s[j];
  }
  if (tid == 0 && bad_s && p.flag[0] == 0) { p.flag[0] = p.code; p.flag[1] = bad_s; }
}

struct SvdFinishP {
  float* Uf;                 // USER factors [n_users, ldu]: Q W, or Z W in the transposed case
  float* Vf;                 // ITEM factors [n_items, ldv]: Z W, or Q W in the transposed case
  int ldu, ldv, n_users, n_items, transposed;
  float* sigma;              // [k]
};

// One workgroup per factor column c.  sigma_c is the norm of column c of Z W (the Rayleigh estimate: second order in the error of w_c,
// where the norm of the Jacobi column carries every rotation's rounding), summed in a fixed order; the transposed case scales
// USER by 1 / sigma and ITEM by sigma; the sign rule negates both columns when the entry of largest magnitude of USER's (first index
// on ties) is negative.
__global__ __launch_bounds__(256) void svd_finish_kernel(SvdFinishP p) {
  __shared__ float red_v[256];
  __shared__ int red_i[256];
  __shared__ float fu_s, fv_s;
  const int c = blockIdx.x, tid = threadIdx.x;
  const float* R = p.transposed ? p.Uf : p.Vf;
  const int nr = p.transposed ? p.n_users : p.n_items, ldr = p.transposed ? p.ldu : p.ldv;
  float s = 0.f;
  for (int r = tid; r < nr; r += 256) { const float v = R[(size_t)r * ldr + c]; s += v * v; }
  red_v[tid] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red_v[tid] += red_v[tid + o];
    __syncthreads();
  }
  const float sg = sqrtf(red_v[0]);
  __syncthreads();
  float bv = -1.f;
  int bi = 0;
  for (int r = tid; r < p.n_users; r += 256) {      // ascending rows: the first index of the largest magnitude
    const float v = fabsf(p.Uf[(size_t)r * p.ldu + c]);
    if (v > bv) { bv = v; bi = r; }
  }
  red_v[tid] = bv; red_i[tid] = bi;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      const float v = red_v[tid + o];
      const int i = red_i[tid + o];
      if (v > red_v[tid] || (v == red_v[tid] && i < red_i[tid])) { red_v[tid] = v; red_i[tid] = i; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float sign = p.Uf[(size_t)red_i[0] * p.ldu + c] < 0.f ? -1.f : 1.f;
    const bool scale = p.transposed && sg > 0.f;
    fu_s = scale ? sign / sg : sign;
    fv_s = scale ? sign * sg : sign;
    p.sigma[c] = sg;
  }
  __syncthreads();
  const float fu = fu_s, fv = fv_s;
  if (fu != 1.f)
    for (int r = tid; r < p.n_users; r += 256) p.Uf[(size_t)r * p.ldu + c] *= fu;
  if (fv != 1.f)
    for (int r = tid; r < p.n_items; r += 256) p.Vf[(size_t)r * p.ldv + c] *= fv;
}

}  // namespace ganmf
