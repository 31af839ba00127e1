// topk_rounds.hpp -- the block-wide arg-max round with removal, written once: the selection rule of recommend() (mask_topk_body,
// kernels.hpp), of the candidate route (cand_topk_body, cand_topk.hpp) and of the item-similarity fits (itemknn_fit_kernel,
// p3_rows_kernel, p3_columns_kernel, slim_rows_kernel).
//
// One round over w[0, n), 256 threads: thread t scans the ids t, t + 256, ... in increasing order and keeps the FIRST maximum it
// meets; a 64-lane xor butterfly and then the four wave slots in LDS are folded with "the larger value, of equal values the smaller
// id".  So ties go to the smaller id at every level, and the winner does not depend on which thread saw it.  The caller removes the
// winner (w[id] = -inf) and runs the next round.  An empty or exhausted row (everything -inf) yields no winner.
#pragma once
#include <hip/hip_runtime.h>

namespace ganmf {

constexpr int TOPK_THREADS = 256;      // the workgroup every caller launches: four waves, four slots

// Every thread of the workgroup: the best of w[0, n) per wave into wv[wave] / wi[wave] (-inf / 0x7fffffff where the wave saw nothing),
// then a barrier.  wv and wi are four LDS slots each.
template <typename T>
__device__ __forceinline__ void block_argmax(const T* w, int n, T* wv, int* wi) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int j = tid; j < n; j += TOPK_THREADS) {
    const T v = w[j];
    if (v > bv) { bv = v; bi = j; }      // strided scan visits ids in increasing order: first max wins
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
  __syncthreads();
}

// Behind block_argmax's barrier, by thread 0 alone or by every thread alike: the four wave slots folded into (*v, *i).
// False: nothing is left in the row.
template <typename T>
__device__ __forceinline__ bool argmax_of_waves(const T* wv, const int* wi, T* v, int* i) {
  T bv = wv[0];
  int bi = wi[0];
#pragma unroll
  for (int q = 1; q < TOPK_THREADS / 64; ++q)
    if (wv[q] > bv || (wv[q] == bv && wi[q] < bi)) { bv = wv[q]; bi = wi[q]; }
  *v = bv;
  *i = bi;
  return bv > -INFINITY && bi != 0x7fffffff;
}

// The topk largest of w[0, n), the NON-ZERO ones stored in descending order, rounded to float: out_idx / out_val[0, *out_cnt).  Called
// by the whole workgroup behind a barrier that follows the last write of w; any_neg (the same in every thread) says whether the row
// holds a negative value.  w is consumed (the picks become -inf); thread 0 stores the picks and the count.  The caller puts a barrier
// in front of the next use of w, wv / wi and s_stop.
template <typename T>
__device__ __forceinline__ void select_topk_nonzero(T* w, int n, int topk, int any_neg, int* out_idx, float* out_val, int* out_cnt,
                                                    T* wv, int* wi, int* s_stop) {
  const int tid = threadIdx.x;
  int cnt = 0;
  for (int t = 0; t < topk; ++t) {
    block_argmax(w, n, wv, wi);
    if (tid == 0) {
      T v;
      int b;
      const bool ok = argmax_of_waves(wv, wi, &v, &b);
      if (ok && v != (T)0) {
        out_idx[cnt] = b;
        out_val[cnt] = (float)v;
        ++cnt;
      }
      if (ok) w[b] = -INFINITY;
      // nothing left, or only zeros left in a row without negative values: no later round stores anything
      *s_stop = (!ok || (v == (T)0 && !any_neg)) ? 1 : 0;
    }
    __syncthreads();
    if (*s_stop) break;
  }
  if (tid == 0) *out_cnt = cnt;
}

}  // namespace ganmf
