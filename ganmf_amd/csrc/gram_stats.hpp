// Cosine similarity of score rows (ganmf_score_similarity): row normalisation, the symmetric Gram product with its statistics in the
// epilogue, and the block means of the heat-map.  The computation under AblationStudy.py:88-92,113-117 of the reference
// (cosine_similarity of all predictions, its mean and standard deviation, the matrix behind the heat-map), on the device.
//
//   * sim_normalize_kernel: one workgroup per score row; sum of squares in float64 in a fixed tree order, the row scaled by the
//     inverse norm in place (one rounding per element), pad columns up to the leading dimension written as zeros (the Gram product
//     consumes them along K).  A row of norm 0 is stored as zeros and flagged (sklearn's normalize divides such a row by 1).
//   * gram kernels: C = S^ . S^T is an NT product of a matrix with itself.  Only the tiles tj >= ti of the 128 x 128 tile grid are
//     formed (gram_tile_coords: a bijection from the 1-D grid onto the upper triangle, row by row, each XCD a contiguous range of
//     the list as in tile_coords), on the K loops of gemm_bf16s_body (exact three-way bf16 split: the default, measured 0.89 ms against
//     1.35 ms at 6040 x 3706, profiles/r07_similarity.md) or gemm_f32_body (plain fp32 MFMA, GANMF_TUNE=gram=0) behind EPI_GRAM_STATS.  The epilogue forms d = c - 1 per element in fp32 (the statistics of interest sit at c ~ 1, where
//     sum(d^2) / n^2 - (sum(d) / n^2)^2 has no cancellation) and reduces sum(d), sum(d^2) of the tile's in-range elements in float64:
//     per thread in row order, lanes by an XOR tree, waves in index order.  One pair per tile goes to an arena; the host adds the
//     pairs in tile order, off-diagonal tiles twice.  No atomics: the same bytes on every call and handle.  The tile and its mirror
//     image are stored only when the caller wants the matrix or its block means.
//   * sim_pool_kernel: block means of the stored matrix, row i in bin floor(i * pool / n); one workgroup per bin, float64 sum in a
//     fixed order.
#pragma once
#include "gemm_bf16s.hpp"

namespace ganmf {

constexpr int GRAM_TILE = 128;

// first list position of tile row ti of the upper triangle of an nt x nt tile grid (rows hold nt, nt - 1, ... tiles)
__host__ __device__ inline long long gram_row_start(int nt, int ti) { return (long long)ti * nt - (long long)ti * (ti - 1) / 2; }

__device__ inline void gram_tile_coords(const GemmP& p, int bid, int nblk, int& tm, int& tn) {
  const int nt = p.tiles_m;
  const long long t = xcd_remap(bid, nblk);
  // ti = the largest row whose start is <= t: closed form, then exact correction of the square root's rounding
  const double b = 2.0 * nt + 1.0;
  int ti = (int)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  ti = max(0, min(ti, nt - 1));
  while (ti + 1 < nt && gram_row_start(nt, ti + 1) <= t) ++ti;
  while (ti > 0 && gram_row_start(nt, ti) > t) --ti;
  tm = ti;
  tn = ti + (int)(t - gram_row_start(nt, ti));
}

// `smem` holds BM * BN floats and is idle.  p.M = p.N = n rows; p.C == nullptr: statistics only.
template <int BM, int BN, int TM, int TN>
__device__ inline void gram_epilogue(const GemmP& p, const f32x16 (&acc)[TM][TN], float* smem, const TileCoord& tc_) {
  static_assert(BM == BN, "the mirror store assumes square tiles");
  constexpr int WM = BM / 2, WN = BN / 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = (wave >> 1) & 1, wc = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int tm = tc_.tm, tn = tc_.tn, m0 = tc_.m0, n0 = tc_.n0;
  const int n = p.M;
  float* __restrict__ ct = smem;      // the tile as a natural [BM][BN] image (gemm_epilogue's staging)
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ct[(wr * WM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * BN + wc * WN + b * 32 + li] = acc[a][b][r];
  __syncthreads();

  constexpr int C4 = BN / 4, RPP = 256 / C4;
  static_assert(BM % RPP == 0, "row pass must cover the tile in whole steps");
  const int tc = tid % C4, tr = tid / C4;
  float* __restrict__ C = p.C;
  double sd = 0.0, sd2 = 0.0;
  const int col = n0 + tc * 4;
#pragma unroll 4
  for (int j = 0; j < BM / RPP; ++j) {
    const int row_l = tr + j * RPP, row = m0 + row_l;
    if (row < n && col < n) {
      float4 v = *reinterpret_cast<const float4*>(ct + row_l * BN + tc * 4);
      if (tm == tn) {      // a diagonal tile holds both c_ij and c_ji: the one above the diagonal stands for both (an exactly symmetric matrix
                           // under the split arithmetic too, whose (hi, lo) and (lo, hi) products enter the sum in a fixed, not a symmetric, order)
        if (row_l > tc * 4) v.x = ct[(tc * 4) * BN + row_l];
        if (row_l > tc * 4 + 1) v.y = ct[(tc * 4 + 1) * BN + row_l];
        if (row_l > tc * 4 + 2) v.z = ct[(tc * 4 + 2) * BN + row_l];
        if (row_l > tc * 4 + 3) v.w = ct[(tc * 4 + 3) * BN + row_l];
      }
      const float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (col + q < n) {
          const float d = o[q] - 1.f;
          sd += (double)d;
          sd2 += (double)d * (double)d;
        }
      if (C) {
        if (col + 3 < n) *reinterpret_cast<float4*>(C + (size_t)row * p.ldc + col) = v;
        else
          for (int q = 0; q < 4 && col + q < n; ++q) C[(size_t)row * p.ldc + col + q] = o[q];
      }
    }
  }
  if (C && tn != tm) {
    // mirror image: row n0 + j of the matrix takes column j of the tile.  tm < tn: every row m0 .. m0 + BM - 1 is in range.
    // (Lanes of a wave read one LDS bank here; the pass exists only when the matrix is wanted, and is ~3 % of the tile's K loop.)
#pragma unroll 4
    for (int j = 0; j < BN / RPP; ++j) {
      const int jl = tr + j * RPP, grow = n0 + jl;
      if (grow < n) {
        const float* q = ct + (tc * 4) * BN + jl;
        *reinterpret_cast<float4*>(C + (size_t)grow * p.ldc + m0 + tc * 4) = make_float4(q[0], q[BN], q[2 * BN], q[3 * BN]);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sd += __shfl_xor(sd, o); sd2 += __shfl_xor(sd2, o); }
  __syncthreads();      // every wave is done reading the staged tile
  double* red = reinterpret_cast<double*>(smem);
  if (lane == 0) { red[2 * wave] = sd; red[2 * wave + 1] = sd2; }
  __syncthreads();
  if (tid == 0) {
    const long long t = gram_row_start(p.tiles_m, tm) + (tn - tm);
    p.epi.gram_partials[2 * t] = (red[0] + red[2]) + (red[4] + red[6]);
    p.epi.gram_partials[2 * t + 1] = (red[1] + red[3]) + (red[5] + red[7]);
  }
}

__global__ __launch_bounds__(256) void gram_f32_kernel(const GemmP p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * (GRAM_TILE + GRAM_TILE) * 32];      // the ring of gemm_f32_mfma<128, 128, 32, 2>
  gemm_f32_body<GRAM_TILE, GRAM_TILE, 32, 2, false, false, 1, true>(p, (int)blockIdx.x, (int)gridDim.x, smem);
}

__global__ __launch_bounds__(256, 2) void gram_bf16x3_kernel(const GemmP p) {
  __shared__ __attribute__((aligned(16))) float smem[Bf16sLds<GRAM_TILE, GRAM_TILE, 32, 3>::DW];
  gemm_bf16s_body<GRAM_TILE, GRAM_TILE, 32, false, false, 3, false, true>(p, (int)blockIdx.x, (int)gridDim.x, smem);
}

// S [gridDim.x, ld]: row r <- row r / ||row r||_2 over its first W columns, columns W .. ld - 1 <- 0; zero_row[r] = (norm == 0)
__global__ __launch_bounds__(256) void sim_normalize_kernel(float* __restrict__ S, int ld, int W, int* __restrict__ zero_row) {
  __shared__ double red[4];
  float* __restrict__ r = S + (size_t)blockIdx.x * ld;
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int c = tid * 4; c < W; c += 1024) {      // (ld is a multiple of 64: a float4 never crosses the row's end)
    const float4 v = *reinterpret_cast<const float4*>(r + c);
    s += (double)v.x * v.x;
    if (c + 1 < W) s += (double)v.y * v.y;
    if (c + 2 < W) s += (double)v.z * v.z;
    if (c + 3 < W) s += (double)v.w * v.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const double total = (red[0] + red[1]) + (red[2] + red[3]);
  const bool zero = !(total > 0.0);
  const double inv = zero ? 0.0 : 1.0 / sqrt(total);
  for (int c = tid * 4; c < ld; c += 1024) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!zero && c < W) {
      const float4 x = *reinterpret_cast<const float4*>(r + c);
      v.x = (float)((double)x.x * inv);
      if (c + 1 < W) v.y = (float)((double)x.y * inv);
      if (c + 2 < W) v.z = (float)((double)x.z * inv);
      if (c + 3 < W) v.w = (float)((double)x.w * inv);
    }
    *reinterpret_cast<float4*>(r + c) = v;
  }
  if (tid == 0) zero_row[blockIdx.x] = zero ? 1 : 0;
}

// first row of bin b: the smallest i with floor(i * pool / n) == b
__host__ __device__ inline int sim_bin_begin(int n, int pool, int b) { return (int)(((long long)b * n + pool - 1) / pool); }

// out[bi, bj] = mean of C[rows of bin bi, rows of bin bj]; grid = pool * pool
__global__ __launch_bounds__(256) void sim_pool_kernel(const float* __restrict__ C, int ldc, int n, int pool, float* __restrict__ out) {
  __shared__ double red[4];
  const int bi = blockIdx.x / pool, bj = blockIdx.x % pool;
  const int r0 = sim_bin_begin(n, pool, bi), r1 = sim_bin_begin(n, pool, bi + 1);
  const int c0 = sim_bin_begin(n, pool, bj), c1 = sim_bin_begin(n, pool, bj + 1);
  const int cols = c1 - c0;
  const long long total = (long long)(r1 - r0) * cols;
  double s = 0.0;
  for (long long i = threadIdx.x; i < total; i += 256) {
    const int r = (int)(i / cols), c = (int)(i % cols);
    s += (double)C[(size_t)(r0 + r) * ldc + c0 + c];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / (double)total);
}

}  // namespace ganmf
