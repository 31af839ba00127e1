// CFGAN's masked row kernels (CFGAN.py:138-172): everything of the step that is neither a dense product nor the discriminator's head.
//   densify   c = URM rows as a dense [nb, ld] block with the bias-folding ones column at N
//   forward   g_out = fake * (c + PM bit) written straight into the discriminator's input block [c | x | 1], plus the row's
//             zero-reconstruction partial sum_j fake^2 * ZR bit -- one read of fake, walking the mask words
//   backward  dfake = (c + PM bit) * dgout + (2 coef / B) * fake * ZR bit
//   sums      sum(theta^2) of a tensor and the step's loss, both in a fixed order (bitwise reproducible)
//   transpose the item-mode score cache
// Wave64, plain C++: one 256-thread workgroup per row, lane j walks columns j, j + 256, ... (coalesced dwords; the 32 lanes of a mask
// word read the same address), sums go lane -> wave shuffle -> four wave totals in wave order.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ganmf {

// sum over the 256 threads of a workgroup, the same value in every thread; red4 is reusable after the call
__device__ __forceinline__ float cfgan_block_sum(float v, float* red4) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// X[b, :] = dense CSR row (rows ? rows[b] : row0 + b), X[b, ncols] = 1, every other column of the padded row 0
__global__ __launch_bounds__(256) void cfgan_densify_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                            const float* __restrict__ data, const int* __restrict__ rows, int row0,
                                                            int ncols, float* __restrict__ X, int ldx) {
  const int b = blockIdx.x;
  const int r = rows ? rows[b] : row0 + b;
  float* x = X + (size_t)b * ldx;
  float4* x4 = reinterpret_cast<float4*>(x);
  for (int c = threadIdx.x; c < ldx / 4; c += 256) x4[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const long long s = indptr[r], e = indptr[r + 1];
  for (long long j = s + threadIdx.x; j < e; j += 256) x[indices[j]] = data[j];
  if (threadIdx.x == 0) x[ncols] = 1.0f;
}

struct CfganRowP {
  const float* C;          // [nb, ld] dense rows
  float* fake;             // [nb, ld] generator output; the backward pass turns it into dfake in place of dgout
  float* dgout;            // [nb, ld] backward: d loss / d g_out in, dfake out
  int ld, ncols, nb, row0;
  const unsigned* pm;      // [rows, words] or nullptr (scheme ZR: the train mask is c)
  const unsigned* zr;      // [rows, words] or nullptr (scheme PM, and the discriminator step)
  int words;
  float* DX;               // [2 nb | nb, ldx]: forward output
  int ldx;
  int d_step;              // 1: rows [0, nb) = [c | c | 1], rows [nb, 2 nb) = [c | g_out | 1];  0: rows [0, nb) = [c | g_out | 1]
  float* zr_part;          // [nb] per-row sum fake^2 * ZR (generator step)
  float zr_scale;          // backward: 2 coef / B
};

__global__ __launch_bounds__(256) void cfgan_mask_fwd_kernel(const CfganRowP p) {
  __shared__ float red[4];
  const int b = blockIdx.x, N = p.ncols;
  const float* __restrict__ c = p.C + (size_t)b * p.ld;
  const float* __restrict__ f = p.fake + (size_t)b * p.ld;
  const unsigned* __restrict__ pm = p.pm ? p.pm + (size_t)(p.row0 + b) * p.words : nullptr;
  const unsigned* __restrict__ zr = p.zr ? p.zr + (size_t)(p.row0 + b) * p.words : nullptr;
  float* __restrict__ xr = p.d_step ? p.DX + (size_t)b * p.ldx : nullptr;            // the real row
  float* __restrict__ xf = p.DX + (size_t)(p.d_step ? p.nb + b : b) * p.ldx;        // the generated row
  float acc = 0.f;
  for (int j = threadIdx.x; j < N; j += 256) {
    const float cv = c[j], fv = f[j];
    const float m = cv + (pm ? (float)((pm[j >> 5] >> (j & 31)) & 1u) : 0.f);
    if (zr && ((zr[j >> 5] >> (j & 31)) & 1u)) acc += fv * fv;
    if (xr) { xr[j] = cv; xr[N + j] = cv; }
    xf[j] = cv;
    xf[N + j] = fv * m;
  }
  if (threadIdx.x == 0) {
    if (xr) xr[2 * N] = 1.0f;
    xf[2 * N] = 1.0f;
  }
  if (p.zr_part) {
    const float t = cfgan_block_sum(acc, red);
    if (threadIdx.x == 0) p.zr_part[b] = t;
  }
}

__global__ __launch_bounds__(256) void cfgan_mask_bwd_kernel(const CfganRowP p) {
  const int b = blockIdx.x, N = p.ncols;
  const float* __restrict__ c = p.C + (size_t)b * p.ld;
  const float* __restrict__ f = p.fake + (size_t)b * p.ld;
  float* __restrict__ d = p.dgout + (size_t)b * p.ld;
  const unsigned* __restrict__ pm = p.pm ? p.pm + (size_t)(p.row0 + b) * p.words : nullptr;
  const unsigned* __restrict__ zr = p.zr ? p.zr + (size_t)(p.row0 + b) * p.words : nullptr;
  for (int j = threadIdx.x; j < N; j += 256) {
    const float m = c[j] + (pm ? (float)((pm[j >> 5] >> (j & 31)) & 1u) : 0.f);
    float v = m * d[j];
    if (zr && ((zr[j >> 5] >> (j & 31)) & 1u)) v += p.zr_scale * f[j];
    d[j] = v;
  }
}

// out[blockIdx.x] = sum of p[i]^2 over the block's float4 slots i = blockIdx.x * 256 + tid, + gridDim.x * 256, ... (pad elements are 0)
constexpr int CFGAN_SQ_BLOCKS = 64;
__global__ __launch_bounds__(256) void cfgan_sumsq_kernel(const float* __restrict__ p, long long n4, float* __restrict__ out) {
  __shared__ float red[4];
  float sq = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 t = reinterpret_cast<const float4*>(p)[i];
    sq += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
  }
  const float s = cfgan_block_sum(sq, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// *out = (sum la + sum lb) / nb + reg / 2 * sum sq + coef * sum zr / nb    (lb, sq, zr may be nullptr); one workgroup
__global__ __launch_bounds__(256) void cfgan_loss_kernel(const float* __restrict__ la, const float* __restrict__ lb, int nb,
                                                         const float* __restrict__ sq, int nsq, float reg,
                                                         const float* __restrict__ zr, float coef, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f, q = 0.f, z = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) {
    a += la[i];
    if (lb) b += lb[i];
    if (zr) z += zr[i];
  }
  if (sq) for (int i = threadIdx.x; i < nsq; i += 256) q += sq[i];
  a = cfgan_block_sum(a, red);
  b = cfgan_block_sum(b, red);
  q = cfgan_block_sum(q, red);
  z = cfgan_block_sum(z, red);
  if (threadIdx.x == 0) {
    const float inv = 1.0f / (float)nb;
    float l = a * inv;
    if (lb) l += b * inv;
    if (sq) l += reg * (0.5f * q);
    if (zr) l += coef * (z * inv);
    *out = l;
  }
}

// dst[j, col0 + b] = src[b, j] for b < nb, j < ncols: 32 x 32 tiles through LDS (256 threads = 32 x 8)
__global__ __launch_bounds__(256) void cfgan_transpose_kernel(const float* __restrict__ src, int lds_, int nb, int ncols,
                                                              float* __restrict__ dst, int ldd, int col0) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  for (int i = ty; i < 32; i += 8) {
    const int b = b0 + i, j = j0 + tx;
    tile[i][tx] = (b < nb && j < ncols) ? src[(size_t)b * lds_ + j] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i, b = b0 + tx;
    if (j < ncols && b < nb) dst[(size_t)j * ldd + col0 + b] = tile[tx][i];
  }
}

}  // namespace ganmf
