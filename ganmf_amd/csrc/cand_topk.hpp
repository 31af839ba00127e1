// cand_topk.hpp -- negative-sample evaluation (Base/Evaluation/Evaluator.py:419-590): score and rank each row's OWN candidate list.
//
// The reference's EvaluatorNegativeItemSample makes one recommend(user, items_to_compute = candidates, return_scores = True) call per
// user: a full-width score row, of which only the user's ~100 candidates (URM_test + URM_test_negative, Evaluator.py:450-452) can be
// recommended.  Here one 256-thread workgroup per requested row r = ids[b] gathers the factor rows of r's candidates, forms only those
// dot products and selects among them; the [n, W] score matrix never exists.
//
//   candidates  c_indices[c_indptr[r] : c_indptr[r + 1]], ascending and unique (ganmf_set_candidates_csr makes them so), at most
//               GANMF_CANDIDATES_MAX_PER_ROW of them: one float score and one int id per candidate live in LDS.
//   scoring     wave w of the four takes the candidates j = w (mod 4), four of them in flight; lanes run along k with 16-byte loads of
//               the candidate's factor row (rows are ld-padded to 64 floats, so every load is whole and aligned); a lane's partial
//               is an fp32 FMA chain in ascending k, the 64 partials are added in a fixed xor-butterfly order.  The row's own factor
//               is held in registers (ld <= 512) or in LDS (longer k), zero from column k on.  No atomics: the same bytes on every run.
//   masks       the rules of mask_topk_body (kernels.hpp): a cold row or an item outside the score filter -> -inf; with remove_seen
//               every seen item of r that is a candidate -> -inf (the candidate list is sorted: binary search per seen item, so the
//               seen row itself need not be sorted).
//   RMSE        (kRmse, ganmf_evaluate_candidates with counts) as mask_topk_rmse_kernel forms it, thread for thread: squared fp32
//               errors over r's test items, finite ones only -- a test item that is no candidate scores -inf under the MF contract's
//               items_to_compute rule and drops out -- NaN without any.
//   selection   `cutoff` rounds of block_argmax (topk_rounds.hpp) with removal over the candidate POSITIONS; ties go to the smaller position =
//               the smaller item id.  Outputs are global item ids and scores, [n, cutoff], padded with -1 / -inf: the layout
//               eval_topk_kernel / eval_topk_full_kernel read.  An exhausted row pads the rest at once and stops.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ganmf_hip.h"
#include "kernels.hpp"

namespace ganmf {

constexpr int CAND_MAX_PER_ROW = GANMF_CANDIDATES_MAX_PER_ROW;
constexpr int CAND_REG_LD = 512;        // longest padded factor row held in registers (two float4 per lane)

struct CandP {
  const float* rows;            // factor matrix of the requested rows (U in user mode, V in item mode), [.., ld]
  const float* cols;            // factor matrix of the candidates, [W, ld]
  int ld, k;
  const int* ids;               // [n] requested rows
  const long long* c_indptr;    // candidate lists, evaluation orientation
  const int* c_indices;
  const long long* seen_indptr; // nullptr: seen items stay
  const int* seen_indices;
  const unsigned char* item_mask;   // nullptr: no item filter
  const long long* cold_indptr;     // nullptr: cold rows are scored
  int cutoff;
  int cap;                      // candidate slots in LDS (>= the longest list of this launch, a multiple of 64)
  int* out_items;               // [n, cutoff]
  float* out_vals;
};

__device__ __forceinline__ float4 cand_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// position of `item` in the ascending list it[0 .. n), -1 when absent
__device__ __forceinline__ int cand_find(const int* it, int n, int item) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (it[mid] < item) lo = mid + 1; else hi = mid;
  }
  return (lo < n && it[lo] == item) ? lo : -1;
}

__device__ __forceinline__ float cand_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// NP float4 per lane cover a padded row of up to NP * 256 floats
template <int NP>
__device__ __forceinline__ void cand_score_regs(const CandP& p, const float* __restrict__ urow, float* s, const int* it, int nc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 u[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int off = q * 256 + lane * 4;
    u[q] = off < p.ld ? cand_ld4(urow + off) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (off + 0 >= p.k) u[q].x = 0.f;
    if (off + 1 >= p.k) u[q].y = 0.f;
    if (off + 2 >= p.k) u[q].z = 0.f;
    if (off + 3 >= p.k) u[q].w = 0.f;
  }
  for (int j0 = wave; j0 < nc; j0 += 16) {
    float4 v[4][NP];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + 4 * c;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int off = q * 256 + lane * 4;
        v[c][q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < nc && off < p.ld) v[c][q] = cand_ld4(p.cols + (size_t)it[j] * p.ld + off);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + 4 * c;
      if (j >= nc) break;
      float acc = 0.f;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        acc = fmaf(u[q].x, v[c][q].x, acc);
        acc = fmaf(u[q].y, v[c][q].y, acc);
        acc = fmaf(u[q].z, v[c][q].z, acc);
        acc = fmaf(u[q].w, v[c][q].w, acc);
      }
      acc = cand_wave_sum(acc);
      if (lane == 0) s[j] = acc;
    }
  }
}

// long k: the row's factor (zero from column k on) sits in LDS behind the candidate slots
__device__ __forceinline__ void cand_score_lds(const CandP& p, const float* __restrict__ urow, float* ul, float* s, const int* it, int nc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < p.ld; i += 256) ul[i] = i < p.k ? urow[i] : 0.f;
  __syncthreads();
  for (int j = wave; j < nc; j += 4) {
    const float* vr = p.cols + (size_t)it[j] * p.ld;
    float acc = 0.f;
    for (int off = lane * 4; off < p.ld; off += 256) {
      const float4 v = cand_ld4(vr + off);
      const float4 u = *reinterpret_cast<const float4*>(ul + off);
      acc = fmaf(u.x, v.x, acc);
      acc = fmaf(u.y, v.y, acc);
      acc = fmaf(u.z, v.z, acc);
      acc = fmaf(u.w, v.w, acc);
    }
    acc = cand_wave_sum(acc);
    if (lane == 0) s[j] = acc;
  }
}

template <bool kRmse>
__device__ __forceinline__ void cand_topk_body(const CandP& p, const RmseP& rp) {
  extern __shared__ __attribute__((aligned(16))) float cand_lds[];
  __shared__ float wv[4];
  __shared__ int wi[4];
  float* s = cand_lds;                                        // [cap] scores
  int* it = reinterpret_cast<int*>(cand_lds + p.cap);         // [cap] item ids
  float* ul = cand_lds + 2 * (size_t)p.cap;                   // [ld] (long k only)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = p.ids[b];
  const long long c0 = p.c_indptr[r];
  const int nc = min((int)(p.c_indptr[r + 1] - c0), p.cap);   // (the host has refused longer lists)
  for (int j = tid; j < nc; j += 256) it[j] = p.c_indices[c0 + j];
  __syncthreads();
  const float* urow = p.rows + (size_t)r * p.ld;
  if (p.ld <= 256) cand_score_regs<1>(p, urow, s, it, nc);
  else if (p.ld <= CAND_REG_LD) cand_score_regs<2>(p, urow, s, it, nc);
  else cand_score_lds(p, urow, ul, s, it, nc);
  __syncthreads();
  // MF contract (Base/BaseMatrixFactorizationRecommender.py:113-119,128-143), as mask_topk_body applies it
  const bool cold = p.cold_indptr != nullptr && p.cold_indptr[r + 1] == p.cold_indptr[r];
  if (p.item_mask != nullptr || cold)
    for (int j = tid; j < nc; j += 256)
      if (cold || !p.item_mask[it[j]]) s[j] = -INFINITY;
  if (p.seen_indptr) {
    const long long s0 = p.seen_indptr[r], s1 = p.seen_indptr[r + 1];
    for (long long j = s0 + tid; j < s1; j += 256) {
      const int pos = cand_find(it, nc, p.seen_indices[j]);
      if (pos >= 0) s[pos] = -INFINITY;
    }
  }
  __syncthreads();
  if (kRmse) {
    __shared__ double rs[4];
    __shared__ int rc[4];
    const long long t0 = rp.t_indptr[r], t1 = rp.t_indptr[r + 1];
    double sq = 0.0;
    int cnt = 0;
    for (long long j = t0 + tid; j < t1; j += 256) {
      const int pos = cand_find(it, nc, rp.t_indices[j]);
      const float d = (pos >= 0 ? s[pos] : -INFINITY) - rp.t_rating[j];
      const float d2 = d * d;
      if (isfinite(d2)) { sq += (double)d2; ++cnt; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sq += __shfl_xor(sq, o);
      cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { rs[wave] = sq; rc[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
      const double t = ((rs[0] + rs[1]) + rs[2]) + rs[3];
      const int c = rc[0] + rc[1] + rc[2] + rc[3];
      rp.out[b] = c > 0 ? (float)sqrt(t / (double)c) : NAN;
    }
  }
  int* oi = p.out_items + (size_t)b * p.cutoff;
  float* ov = p.out_vals + (size_t)b * p.cutoff;
  for (int t = 0; t < p.cutoff; ++t) {
    block_argmax(s, nc, wv, wi);
    float v;
    int i;
    const bool ok = argmax_of_waves(wv, wi, &v, &i);      // every thread folds the slots: the same for every thread
    if (!ok) {
      for (int t2 = t + tid; t2 < p.cutoff; t2 += 256) { oi[t2] = -1; ov[t2] = -INFINITY; }
      break;
    }
    if (tid == 0) {
      oi[t] = it[i];
      ov[t] = v;
      s[i] = -INFINITY;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void cand_topk_kernel(const CandP p) { cand_topk_body<false>(p, RmseP{}); }
__global__ __launch_bounds__(256) void cand_topk_rmse_kernel(const CandP p, const RmseP rp) { cand_topk_body<true>(p, rp); }

}  // namespace ganmf
