// CAAE's samplers (CAAE.py:220,244,270-293,312-321), all counter-based in the manner of cfgan_masks.hpp: every draw is a pure function
// of (seed, epoch, stream, pass / step, index), so nothing depends on the grid, the workgroup size or the order in which anything runs.
//     base  = draw_mix(draw_mix(draw_mix(draw_mix(seed) ^ epoch) ^ stream) ^ step)
//     word  = draw_mix(base ^ index)
//   (a) the epoch's order of the nnz stored interactions: position t holds CSR position caae_perm_index(base, nnz, t), a keyed
//       bijection of [0, nnz) -- a balanced Feistel network of CAAE_FEISTEL_ROUNDS rounds over the smallest even number of bits that
//       covers nnz, walked until it lands below nnz (cycle walking: a bijection of the power-of-two domain restricted to [0, nnz) is a
//       bijection of [0, nnz)).  No sort and no state: any position is computed on its own.
//   (b) one uniform a = (word >> 40) * 2^-24 in [0, 1) per (pass, generator, position); the negative is the first index of the user's CDF
//       row whose value is >= a, clamped to I - 1 (cython_utils.pyx:166-181)
//   (c) m distinct users: the first m values of bijection (a) over [0, U); m users with replacement: ((word >> 32) * U) >> 32
//   (d) the weighted subset Nu of a row's non-interactions: the k smallest Efraimidis-Spirakis keys -log(u) / w, w = exp(r'), u =
//       ((word >> 40) + 0.5) * 2^-24 -- successive sampling without replacement, the distribution of numpy's choice(p=, replace=False).
//       The keys are non-negative floats, so their bit patterns order as they do: subset_select.hpp's selection over those 32 bits, with the
//       tie rule (smaller column first) and the bit plane layout (pack_mask_rows') of CFGAN's masks.
//   (e) n_s CDF draws per batch row under rule (b), index = row * n_s + draw
#pragma once
#include <hip/hip_runtime.h>

#include "counter_draw.hpp"
#include "subset_select.hpp"

namespace ganmf {

enum CaaeStream : unsigned {
  CAAE_S_PERM = 0, CAAE_S_NEG = 1 /* + which */, CAAE_S_USERS = 3 /* + which */, CAAE_S_NU = 5, CAAE_S_ITEMS = 6 /* + which */
};
constexpr int CAAE_FEISTEL_ROUNDS = 6;

__host__ __device__ __forceinline__ unsigned long long caae_base(unsigned long long seed, unsigned long long epoch, unsigned stream,
                                                                 unsigned long long step) {
  return draw_mix(draw_mix(draw_mix(draw_mix(seed) ^ epoch) ^ (unsigned long long)stream) ^ step);
}
__host__ __device__ __forceinline__ unsigned caae_u24(unsigned long long base, unsigned long long index) {
  return (unsigned)(draw_mix(base ^ index) >> 40);
}

// position t of the keyed bijection of [0, n), n >= 1
__host__ __device__ __forceinline__ unsigned long long caae_perm_index(unsigned long long base, unsigned long long n, unsigned long long t) {
  int half = 1;
  while ((1ull << (2 * half)) < n) ++half;
  const unsigned long long mask = (1ull << half) - 1ull;
  unsigned long long x = t;
  do {
    unsigned long long l = x >> half, r = x & mask;
    for (int q = 0; q < CAAE_FEISTEL_ROUNDS; ++q) {
      const unsigned long long f = draw_mix(base ^ (((unsigned long long)(q + 1) << 40) | r)) & mask;
      const unsigned long long nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << half) | r;
  } while (x >= n);
  return x;
}

// first index of the non-decreasing row whose value is >= a, clamped to n - 1
__device__ __forceinline__ int caae_cdf_search(const float* __restrict__ row, int n, float a) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] < a) lo = mid + 1; else hi = mid;
  }
  return min(lo, n - 1);
}

// iu[e] = row of CSR position e
__global__ __launch_bounds__(256) void caae_rows_of_kernel(const long long* __restrict__ indptr, int rows, int* __restrict__ iu) {
  const int r = blockIdx.x;
  if (r >= rows) return;
  for (long long e = indptr[r] + threadIdx.x; e < indptr[r + 1]; e += 256) iu[e] = r;
}

// (a): perm[t], and the user and the item of position t
__global__ __launch_bounds__(256) void caae_perm_kernel(unsigned long long base, long long nnz, const int* __restrict__ iu,
                                                        const int* __restrict__ indices, int* __restrict__ perm, int* __restrict__ tu,
                                                        int* __restrict__ ti) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < nnz; t += (long long)gridDim.x * 256) {
    const long long e = (long long)caae_perm_index(base, (unsigned long long)nnz, (unsigned long long)t);
    perm[t] = (int)e;
    tu[t] = iu[e];
    ti[t] = indices[e];
  }
}

// (b) and (e): out[t] = draw of index t in row (rows ? rows[t] : t / per_row) of the CDF array
__global__ __launch_bounds__(256) void caae_cdf_draw_kernel(unsigned long long base, long long count, const int* __restrict__ rows,
                                                            int per_row, const float* __restrict__ cdf, int ld, int ncols,
                                                            int* __restrict__ out) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < count; t += (long long)gridDim.x * 256) {
    const long long r = rows ? (long long)rows[t] : t / per_row;
    const float a = (float)caae_u24(base, (unsigned long long)t) * 0x1p-24f;
    out[t] = caae_cdf_search(cdf + (size_t)r * ld, ncols, a);
  }
}

// (c)
__global__ __launch_bounds__(256) void caae_users_kernel(unsigned long long base, int m, int U, int distinct, int* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= m) return;
  out[b] = distinct ? (int)caae_perm_index(base, (unsigned long long)U, (unsigned long long)b)
                    : (int)(((draw_mix(base ^ (unsigned long long)b) >> 32) * (unsigned long long)U) >> 32);
}

// (d)
struct CaaeNuP {
  const long long* indptr;      // canonical CSR of the training rows
  const int* indices;
  const int* users;             // [nb] the batch's rows
  const int* k_rows;            // [U] subset size per user (clamped to the row's non-interactions)
  const float* Rp;              // [nb, ld] G'(profile) of the batch's rows: the weights are exp of it
  int ld, ncols, words;
  unsigned long long base;
  unsigned* planes;             // [nb][words]
};

__device__ __forceinline__ unsigned caae_nu_key(unsigned long long base, unsigned row, unsigned col, float r) {
  const float u = ((float)caae_u24(base, ((unsigned long long)row << 32) | col) + 0.5f) * 0x1p-24f;
  return __float_as_uint(fabsf(__logf(u)) / __expf(r));
}

__global__ __launch_bounds__(256) void caae_nu_kernel(const CaaeNuP p) {
  const int b = blockIdx.x;
  const int r = p.users[b];
  unsigned* __restrict__ out = p.planes + (size_t)b * p.words;
  const float* __restrict__ rp = p.Rp + (size_t)b * p.ld;
  const long long s = p.indptr[r], e = p.indptr[r + 1];
  const int n = p.ncols - (int)(e - s);
  const int k = min(max(p.k_rows[r], 0), n);
  if (k == 0) {      // uniform over the workgroup, in front of the selector's first barrier
    for (int w = threadIdx.x; w < p.words; w += 256) out[w] = 0u;
    return;
  }
  subset_select_row(p.indices, s, e, p.ncols, p.words, k, out, [&](int j) { return caae_nu_key(p.base, (unsigned)r, (unsigned)j, rp[j]); });
}

}  // namespace ganmf
