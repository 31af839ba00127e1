// CFGAN's per-epoch mask sampler (CFGAN.py:230: compute_masks): for every training row a uniform random subset of k of its n
// non-interactions, as one bit plane [rows, ceil(I / 32)] of 32-bit words, bit j & 31 of word j >> 5 = column j
// (np.packbits(..., bitorder='little') over 32-bit little-endian words).
//
// Every eligible column j of row r (j not stored in the row's sorted CSR) gets the 32-bit key
//     key(j) = slim_mix(base ^ (r << 32 | j)) >> 32,     base = slim_mix(slim_mix(slim_mix(seed) ^ epoch) ^ plane)
// and the chosen set is the k smallest (key, column) pairs: ties go to the smaller column.  The result is a pure function of
// (seed, epoch, plane, row): nothing depends on the grid, the workgroup size or the order in which anything runs.
//
// One 256-thread workgroup per (row, plane).  The k-th key is found by a 4 x 8-bit radix select from the top byte down: a 256-bin LDS
// histogram of the next byte over the keys that share the prefix found so far (integer LDS atomics: a count does not depend on the
// order of its increments), an inclusive scan of the bins (wave shuffles, then the four wave totals in wave order), and the one bin
// whose range holds the k-th key narrows the prefix.  Keys are recomputed in every pass and none is stored, so any I fits.  The last
// pass walks the columns 256 at a time in ascending order; ties at the threshold key are ranked by wave ballots and a running count
// (order matters there: no atomics), and lane 0 / lane 32 of every wave store the wave's two words.  Columns >= I and profile columns
// never set a bit, so tail bits and profile positions are 0.
#pragma once
#include <hip/hip_runtime.h>

#include "slim_bpr.hpp"

namespace ganmf {

constexpr int CFGAN_PLANE_ZR = 0, CFGAN_PLANE_PM = 1;

__host__ __device__ __forceinline__ unsigned long long cfgan_mask_base(unsigned long long seed, unsigned long long epoch, unsigned plane) {
  return slim_mix(slim_mix(slim_mix(seed) ^ epoch) ^ (unsigned long long)plane);
}
__host__ __device__ __forceinline__ unsigned cfgan_mask_key(unsigned long long base, unsigned row, unsigned col) {
  return (unsigned)(slim_mix(base ^ (((unsigned long long)row << 32) | col)) >> 32);
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

// is column j stored in the sorted index range [s, e)?
__device__ __forceinline__ bool cfgan_in_profile(const int* __restrict__ idx, long long s, long long e, int j) {
  while (s < e) {
    const long long m = (s + e) >> 1;
    const int v = idx[m];
    if (v == j) return true;
    if (v < j) s = m + 1; else e = m;
  }
  return false;
}

__global__ __launch_bounds__(256) void cfgan_masks_kernel(const CfganMaskP p) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wtot[4];
  __shared__ unsigned sel[2];      // the chosen byte, the keys still to take inside it
  const int r = blockIdx.x;
  const int plane = p.plane0 + (int)blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* __restrict__ out = p.planes + ((size_t)plane * p.rows + r) * p.words;
  const long long s = p.indptr[r], e = p.indptr[r + 1];
  const int n = p.ncols - (int)(e - s);
  const int k = min(max(p.k_rows[r], 0), n);
  if (k == 0) {
    for (int w = tid; w < p.words; w += 256) out[w] = 0u;
    return;
  }
  const unsigned long long base = cfgan_mask_base(p.seed, p.epoch, (unsigned)plane);
  unsigned prefix = 0, left = (unsigned)k;      // the k-th smallest key starts with `prefix`; `left` of the keys under it are still wanted
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0u;
    __syncthreads();
    for (int j = tid; j < p.ncols; j += 256) {
      if (cfgan_in_profile(p.indices, s, e, j)) continue;
      const unsigned key = cfgan_mask_key(base, (unsigned)r, (unsigned)j);
      if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned c = hist[tid];
    unsigned incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wtot[w];
    incl += before;
    const unsigned excl = incl - c;
    if (excl < left && left <= incl) { sel[0] = (unsigned)tid; sel[1] = left - excl; }      // exactly one bin: 1 <= left <= eligible keys under the prefix
    __syncthreads();
    prefix |= sel[0] << shift;
    left = sel[1];
    __syncthreads();
  }
  // prefix = the k-th smallest key; `left` >= 1 of the keys equal to it are taken, smallest columns first
  unsigned taken = 0;      // threshold-key columns met so far (uniform over the workgroup)
  const int span = (p.ncols + 255) & ~255;
  for (int j0 = 0; j0 < span; j0 += 256) {
    const int j = j0 + tid;
    bool below = false, tie = false;
    if (j < p.ncols && !cfgan_in_profile(p.indices, s, e, j)) {
      const unsigned key = cfgan_mask_key(base, (unsigned)r, (unsigned)j);
      below = key < prefix;
      tie = key == prefix;
    }
    const unsigned long long tb = __ballot(tie);
    if (lane == 0) wtot[wave] = (unsigned)__popcll(tb);
    __syncthreads();
    unsigned rank = taken + (unsigned)__popcll(tb & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wtot[w];
    taken += (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
    const bool on = below || (tie && rank < left);
    const unsigned long long ob = __ballot(on);
    const int word = (j0 >> 5) + 2 * wave + (lane >> 5);      // lane 0: the wave's columns 0..31, lane 32: its columns 32..63
    if ((lane & 31) == 0 && word < p.words) out[word] = (unsigned)(ob >> (lane & 32));
    __syncthreads();
  }
}

}  // namespace ganmf
