// The subset selector CFGAN's mask sampler (cfgan_masks.hpp) and CAAE's weighted subset Nu (caae_sample.hpp) share: of the columns of
// one row that are not stored in the row's sorted CSR, the k with the smallest (key, column) pairs -- ties go to the smaller column --
// as one row of a bit plane of 32-bit words, bit j & 31 of word j >> 5 = column j (np.packbits(..., bitorder='little') over 32-bit
// little-endian words).  The caller supplies the 32-bit key of a column as a pure function of the column, so the result depends on
// nothing else: not on the grid, the workgroup size or the order in which anything runs.
//
// One 256-thread workgroup per row.  The k-th key is found by a 4 x 8-bit radix select from the top byte down: a 256-bin LDS
// histogram of the next byte over the keys that share the prefix found so far (integer LDS atomics: a count does not depend on the
// order of its increments), an inclusive scan of the bins (wave shuffles, then the four wave totals in wave order), and the one bin
// whose range holds the k-th key narrows the prefix.  Keys are recomputed in every pass and none is stored, so any I fits.  The last
// pass walks the columns 256 at a time in ascending order; ties at the threshold key are ranked by wave ballots and a running count
// (order matters there: no atomics), and lane 0 / lane 32 of every wave store the wave's two words.  Columns >= I and profile columns
// never set a bit, so tail bits and profile positions are 0.
#pragma once
#include <hip/hip_runtime.h>

namespace ganmf {

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

// out[0 .. words) = the plane row of the k smallest (key(j), j) over the columns j < ncols outside indices[s, e).  Called by all 256
// threads of the workgroup with 1 <= k <= the number of such columns (every thread meets the same barriers: a workgroup whose k is 0
// clears its row and leaves before it gets here); key(j) -> unsigned.
template <class Key>
__device__ __forceinline__ void subset_select_row(const int* __restrict__ indices, long long s, long long e, int ncols, int words, int k,
                                                  unsigned* __restrict__ out, Key key) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wtot[4];
  __shared__ unsigned sel[2];      // the chosen byte, the keys still to take inside it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned prefix = 0, left = (unsigned)k;      // the k-th smallest key starts with `prefix`; `left` of the keys under it are still wanted
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0u;
    __syncthreads();
    for (int j = tid; j < ncols; j += 256) {
      if (cfgan_in_profile(indices, s, e, j)) continue;
      const unsigned kj = key(j);
      if (pass == 0 || (kj >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(kj >> shift) & 255u], 1u);
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
  const int span = (ncols + 255) & ~255;
  for (int j0 = 0; j0 < span; j0 += 256) {
    const int j = j0 + tid;
    bool below = false, tie = false;
    if (j < ncols && !cfgan_in_profile(indices, s, e, j)) {
      const unsigned kj = key(j);
      below = kj < prefix;
      tie = kj == prefix;
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
    if ((lane & 31) == 0 && word < words) out[word] = (unsigned)(ob >> (lane & 32));
    __syncthreads();
  }
}

}  // namespace ganmf
