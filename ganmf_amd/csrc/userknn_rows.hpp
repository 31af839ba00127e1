// userknn_rows.hpp -- user-based nearest neighbours on the device: the scoring product W_sparse[users] . URM_train of the reference's
// user-based models (Base/BaseSimilarityMatrixRecommender.py:95-117).  The fit is itemknn_fit_kernel (itemknn_rows.hpp) with the two
// sides of the URM exchanged; the host turns its by-target result into rows (abi_userknn.inc).
//
// Scores: out[r, i] = sum over the stored neighbours v of user u_r of W[u_r, v] R[v, i] -- a weighted sum of the neighbours' profile
// rows.  One workgroup per scored row keeps the dense accumulator of that row: in LDS up to KNN_SCORE_LDS items, above in the row of
// `out` itself.  Each of the workgroup's four waves owns one contiguous range of items, for the whole row: it zeroes the range, walks
// ALL neighbours in stored (ascending) order, takes from each neighbour's sorted profile the entries inside its range (a binary search
// finds the first) and writes the range out.  Inside one neighbour the lanes of a wave touch distinct items (a profile has no
// repeats); between two neighbours the wave's own memory operations stay in program order, and every loop bound is the same in all
// lanes.  So there is no barrier, no atomic, and every stored score is one fp32 FMA chain over ascending neighbours that starts at 0:
// an item no neighbour rated stores 0.f.  The result of a row depends on that row of W and on R alone -- not on the batch, the row's
// place in it or the grid.
// A row of W is NOT bounded by topK (W is selected by column and read by row): lengths and offsets are long long.
#pragma once
#include <hip/hip_runtime.h>
#include "itemknn_rows.hpp"

namespace ganmf {

constexpr int USERKNN_WAVES = KNN_THREADS / 64;

struct UserKnnScoreP {
  const long long* r_indptr;   // side 0: users x items (the weighted URM), items ascending without repeats inside a user
  const int* r_items;
  const float* r_val;
  const long long* w_indptr;   // W by row: row u = the users v with W[u, v] stored, ascending
  const int* w_nbr;
  const float* w_val;
  const int* ids;              // [n] scored users
  int n, n_items;
  int acc_lds;                 // 1: the accumulator is the dynamic LDS (n_items floats); 0: the row of out
  float* out;                  // [n, ldo]
  int ldo;
};

// grid (n): workgroup r scores user ids[r]
__global__ __launch_bounds__(KNN_THREADS) void userknn_score_kernel(const UserKnnScoreP p) {
  extern __shared__ __attribute__((aligned(16))) float uknn_acc[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x, u = p.ids[r];
  float* const row = p.out + (size_t)r * p.ldo;
  float* const acc = p.acc_lds ? uknn_acc : row;
  // the wave's items [lo, hi): a quarter of the catalogue, rounded up to whole 64-item lines
  const int span = ((p.n_items + USERKNN_WAVES - 1) / USERKNN_WAVES + 63) & ~63;
  const long long lo_ll = (long long)wave * span;
  if (lo_ll >= p.n_items) return;
  const int lo = (int)lo_ll, hi = (int)(lo_ll + span < p.n_items ? lo_ll + span : p.n_items);
  for (int i = lo + lane; i < hi; i += 64) acc[i] = 0.f;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const long long we = p.w_indptr[u + 1];
  for (long long q = p.w_indptr[u]; q < we; ++q) {
    const int v = p.w_nbr[q];
    const float wv = p.w_val[q];
    const long long re = p.r_indptr[v + 1];
    // every lane evaluates the same bounds: the first entry of v's profile inside the range, then 64 entries at a time while the
    // first of them is still inside
    for (long long eb = lo == 0 ? p.r_indptr[v] : knn_lower_bound(p.r_items, p.r_indptr[v], re, lo); eb < re && p.r_items[eb] < hi;
         eb += 64) {
      const long long e = eb + lane;
      if (e < re) {
        const int it = p.r_items[e];
        if (it < hi) acc[it] = fmaf(wv, p.r_val[e], acc[it]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (no instruction: the next neighbour's reads follow these writes)
  }
  if (p.acc_lds)
    for (int i = lo + lane; i < hi; i += 64) row[i] = acc[i];
}

}  // namespace ganmf
