// CFGAN's per-epoch mask sampler (CFGAN.py:230: compute_masks): for every training row a uniform random subset of k of its n
// non-interactions, as one bit plane [rows, ceil(I / 32)] of 32-bit words, bit j & 31 of word j >> 5 = column j
// (np.packbits(..., bitorder='little') over 32-bit little-endian words).
//
// Every eligible column j of row r (j not stored in the row's sorted CSR) gets the 32-bit key
//     key(j) = draw_mix(base ^ (r << 32 | j)) >> 32,     base = draw_mix(draw_mix(draw_mix(seed) ^ epoch) ^ plane)
// and the chosen set is the k smallest (key, column) pairs: ties go to the smaller column.  The result is a pure function of
// (seed, epoch, plane, row): nothing depends on the grid, the workgroup size or the order in which anything runs.
//
// One 256-thread workgroup per (row, plane); the selection itself is subset_select.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include "counter_draw.hpp"
#include "subset_select.hpp"

namespace ganmf {

constexpr int CFGAN_PLANE_ZR = 0, CFGAN_PLANE_PM = 1;

__host__ __device__ __forceinline__ unsigned long long cfgan_mask_base(unsigned long long seed, unsigned long long epoch, unsigned plane) {
  return draw_mix(draw_mix(draw_mix(seed) ^ epoch) ^ (unsigned long long)plane);
}
__host__ __device__ __forceinline__ unsigned cfgan_mask_key(unsigned long long base, unsigned row, unsigned col) {
  return (unsigned)(draw_mix(base ^ (((unsigned long long)row << 32) | col)) >> 32);
}

struct CfganMaskP {
  const long long* indptr;      // canonical CSR of the training rows
  const int* indices;
  const int* k_rows;            // [rows] subset size of every row (clamped to the row's non-interactions)
  int rows, ncols, words;       // words = ceil(ncols / 32)
  unsigned long long seed, epoch;
  unsigned* planes;             // [2][rows][words]
  int plane0;                   // plane of blockIdx.y == 0 (a one-plane scheme draws blockIdx.y == 0 only)
};

__global__ __launch_bounds__(256) void cfgan_masks_kernel(const CfganMaskP p) {
  const int r = blockIdx.x;
  const int plane = p.plane0 + (int)blockIdx.y;
  unsigned* __restrict__ out = p.planes + ((size_t)plane * p.rows + r) * p.words;
  const long long s = p.indptr[r], e = p.indptr[r + 1];
  const int n = p.ncols - (int)(e - s);
  const int k = min(max(p.k_rows[r], 0), n);
  if (k == 0) {      // uniform over the workgroup, in front of the selector's first barrier
    for (int w = threadIdx.x; w < p.words; w += 256) out[w] = 0u;
    return;
  }
  const unsigned long long base = cfgan_mask_base(p.seed, p.epoch, (unsigned)plane);
  subset_select_row(p.indices, s, e, p.ncols, p.words, k, out, [&](int j) { return cfgan_mask_key(base, (unsigned)r, (unsigned)j); });
}

}  // namespace ganmf
