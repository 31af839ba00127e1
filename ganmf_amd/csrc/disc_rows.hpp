// Discriminator inference for an arbitrary row list (ganmf_discriminate): what the reference's autoencoder_codes() computes
// (GANMF.py:304-307) and, per row instead of per batch, the EBGAN energy under its discriminator loss (GANMF.py:62-70); for
// DisGANMF the input block of its layer products and the logit (DisGANMF.py:57-65).
//
//   * csr_encode_rows_kernel: E[b, :] = be + sum_j data[j] * We[idx[j], :] for the CSR rows rows[b] -- csr_rowsum_body
//     (kernels.hpp), the row-sum the generator step's sparse front runs, without the embedding gather and without opening an
//     optimizer step.  An empty row gives exactly be.
//   * rowsq kernel: the decode product R = [E | 1] . Wd_ext on the K loop of gemm_bf16s_body (exact three-way bf16 split, unsplit
//     along K) behind rowsq_epilogue: d = acc - inp[m, n] per element in fp32 -- inp a dense block (generated rows) or the CSR
//     lookup csr_quad (real rows; subtracting 0.0f is exact) -- and per row the float64 sum of d^2 over the tile's in-range
//     columns: a thread adds its four columns in column order, the 32 lanes of a row by an XOR tree.  One partial per
//     (row, column tile); R is never stored.  rowsq_finish_kernel adds a row's partials in tile order and divides by N.
//     No atomics: the same bytes on every call and handle.
//   * DisGANMF: disc_densify_kernel expands CSR rows into the block, disc_cols_kernel writes the ones and float(uid) columns,
//     disc_logit_kernel forms [a | 1] . wo_ext per row with dis_head_kernel's summation.
#pragma once
#include "gemm_bf16s.hpp"
#include "kernels.hpp"

namespace ganmf {

constexpr int ROWSQ_TILE = 128;

__global__ __launch_bounds__(256) void csr_encode_rows_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                              const float* __restrict__ data, const int* __restrict__ rows,
                                                              const float* __restrict__ We, int lde, int ncols, int e,
                                                              float* __restrict__ E) {
  __shared__ float4 part[256];
  const int b = blockIdx.x, r = rows[b];
  csr_rowsum_body(indices, data, indptr[r], indptr[r + 1], We, lde, ncols, e, E + (size_t)b * lde, part);
}

// `smem` holds BM * BN floats and is idle.  p.epi: aux (dense input block, ldaux) or csr_* (rows of the block), gram_partials =
// the [M, tiles_n] float64 partials.
template <int BM, int BN, int TM, int TN>
__device__ inline void rowsq_epilogue(const GemmP& p, const f32x16 (&acc)[TM][TN], float* smem, const TileCoord& tc_) {
  constexpr int WM = BM / 2, WN = BN / 2;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = (wave >> 1) & 1, wc = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int tn = tc_.tn, m0 = tc_.m0, n0 = tc_.n0;
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
  static_assert(C4 == 32, "a row of the tile is summed by one 32-lane half of a wave");
  static_assert(BM % RPP == 0, "row pass must cover the tile in whole steps");
  const EpiD& e = p.epi;
  const int tc = tid % C4, tr = tid / C4;
  const int col = n0 + tc * 4;
#pragma unroll 4
  for (int j = 0; j < BM / RPP; ++j) {
    const int row_l = tr + j * RPP, row = m0 + row_l;
    double s = 0.0;
    if (row < p.M && col < p.N) {
      const float4 v = *reinterpret_cast<const float4*>(ct + row_l * BN + tc * 4);
      // (col is a multiple of four below a leading dimension that is one: the float4 stays inside the row; the columns
      // N .. of the block -- its ones column, pads -- are read and never counted)
      const float4 x = e.csr_indptr ? csr_quad(e, row, col) : *reinterpret_cast<const float4*>(e.aux + (size_t)row * e.ldaux + col);
      const float d[4] = {v.x - x.x, v.y - x.y, v.z - x.z, v.w - x.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (col + q < p.N) s += (double)d[q] * (double)d[q];
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);      // (stays inside the row's 32 lanes)
    if (tc == 0 && row < p.M) e.gram_partials[(size_t)row * p.tiles_n + tn] = s;
  }
}

__global__ __launch_bounds__(256, 2) void rowsq_bf16x3_kernel(const GemmP p) {
  __shared__ __attribute__((aligned(16))) float smem[Bf16sLds<ROWSQ_TILE, ROWSQ_TILE, 32, 3>::DW];
  gemm_bf16s_body<ROWSQ_TILE, ROWSQ_TILE, 32, false, true, 3, false, false, true>(p, (int)blockIdx.x, (int)gridDim.x, smem);
}

// value[r] = (partials[r, 0] + partials[r, 1] + ...) / ncols, tiles in index order
__global__ __launch_bounds__(256) void rowsq_finish_kernel(const double* __restrict__ partials, int n, int tiles_n, int ncols,
                                                           double* __restrict__ value) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double s = 0.0;
  for (int t = 0; t < tiles_n; ++t) s += partials[(size_t)r * tiles_n + t];
  value[r] = s / (double)ncols;
}

// X[b, 0 .. ldx) = CSR row rows[b] expanded (pad columns zero); one workgroup per row
__global__ __launch_bounds__(256) void disc_densify_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                           const float* __restrict__ data, const int* __restrict__ rows,
                                                           float* __restrict__ X, int ldx) {
  const int b = blockIdx.x, r = rows[b];
  float* x = X + (size_t)b * ldx;
  for (int c = threadIdx.x; c < ldx / 4; c += 256) reinterpret_cast<float4*>(x)[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const long long s = indptr[r], en = indptr[r + 1];
  for (long long j = s + threadIdx.x; j < en; j += 256) x[indices[j]] = data[j];
}

// the bias-folding ones column of a block, and (uid_col >= 0) DisGANMF's float(uid) column (DisGANMF.py:59,110-111)
__global__ __launch_bounds__(256) void disc_cols_kernel(float* __restrict__ X, int ld, int n, int ones_col, int uid_col,
                                                        const int* __restrict__ rows, int row_offset) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  X[(size_t)b * ld + ones_col] = 1.0f;
  if (uid_col >= 0) X[(size_t)b * ld + uid_col] = (float)(row_offset + rows[b]);
}

// One wave per row: logit = [feat | 1] . wo_ext, summed as dis_head_kernel sums it (kernels.hpp)
__global__ __launch_bounds__(256) void disc_logit_kernel(const float* __restrict__ feat, int ld, int e1, const float* __restrict__ wo,
                                                         int n, double* __restrict__ value) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
#pragma unroll 8
  for (int j = lane; j < e1; j += 64) s += feat[(size_t)r * ld + j] * wo[j];
  s = wave_sum(s);
  if (lane == 0) value[r] = (double)s;
}

}  // namespace ganmf
