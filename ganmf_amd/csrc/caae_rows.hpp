// CAAE's row kernels (CAAE.py:47-119,228-241): everything of an epoch that is neither a dense product nor a draw.
//   cdf rows   softmax of a block of generator outputs r (sigmoid outputs already) as an inclusive prefix sum per row, and the row's
//              log sum exp(r): the CDF the negatives and the policy items are drawn from
//   D-step     per triple (u, i, j): the gathered rows of P and Q, the logit, the coefficient c_t = -(1 - sigmoid(x_t)) / B and the loss
//              parts; then per touched row of P, Q and b one wave that sums the row's contributions in ascending batch position
//              (positives in front of negatives for an item) at the gathered, pre-step values and applies plain SGD.  No floating-point
//              atomics anywhere: a run is bit-reproducible.
//   reward     log sigmoid(+-(<P_u, Q_j> + b_j - 1)) per draw, as min(y, 0) - log1p(exp(-|y|))
//   policy     per batch row dz of the output layer from the draws, the rewards, r, log sum exp(r), the profile and the Nu plane, and
//              the row's loss parts
//   sgd        theta -= lr * (g + beta * theta)
// Wave64, plain C++: one 256-thread workgroup per row (or one wave per triple / draw / touched row), sums go lane -> wave shuffle ->
// four wave totals in wave order (cfgan_block_sum).
#pragma once
#include <hip/hip_runtime.h>

#include "cfgan_rows.hpp"

namespace ganmf {

// ---- CDF rows ---------------------------------------------------------------------------------------------------------------------
// One workgroup per row, tiles of 256 x 16 columns through LDS: thread t owns 16 consecutive columns of the tile (LDS pitch 17: no two
// lanes of a 32-lane group on one bank), sums them one after the other, and thread 0 chains the 256 thread totals onto the carry of the
// tiles before.  A value is fl(offset + local prefix): local prefixes of non-negative terms never decrease, fl is monotone, and the
// offset of thread t + 1 IS the last value of thread t -- so the row is non-decreasing exactly, which the binary search relies on.
constexpr int CAAE_CPT = 16, CAAE_TILE = 256 * CAAE_CPT;

__global__ __launch_bounds__(256) void caae_cdf_rows_kernel(const float* __restrict__ R, int ldr, int ncols, float* __restrict__ cdf,
                                                            int ldc, float* __restrict__ lse) {
  __shared__ float buf[256 * (CAAE_CPT + 1)];
  __shared__ float tot[256];
  __shared__ float off[257];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ r = R + (size_t)b * ldr;
  float a = 0.f;
  for (int j = tid; j < ncols; j += 256) a += expf(r[j]);
  const float S = cfgan_block_sum(a, red);
  if (tid == 0 && lse) lse[b] = logf(S);
  if (!cdf) return;
  float* __restrict__ out = cdf + (size_t)b * ldc;
  float carry = 0.f;
  for (int j0 = 0; j0 < ncols; j0 += CAAE_TILE) {
    for (int i = tid; i < CAAE_TILE; i += 256) {
      const int j = j0 + i;
      buf[(i / CAAE_CPT) * (CAAE_CPT + 1) + (i % CAAE_CPT)] = j < ncols ? expf(r[j]) / S : 0.f;
    }
    __syncthreads();
    float run = 0.f;
#pragma unroll
    for (int q = 0; q < CAAE_CPT; ++q) {
      run += buf[tid * (CAAE_CPT + 1) + q];
      buf[tid * (CAAE_CPT + 1) + q] = run;
    }
    tot[tid] = run;
    __syncthreads();
    if (tid == 0) {
      float o = carry;
      for (int t = 0; t < 256; ++t) { off[t] = o; o += tot[t]; }
      off[256] = o;
    }
    __syncthreads();
    carry = off[256];
    for (int i = tid; i < CAAE_TILE; i += 256) {
      const int j = j0 + i;
      if (j < ncols) out[j] = off[i / CAAE_CPT] + buf[(i / CAAE_CPT) * (CAAE_CPT + 1) + (i % CAAE_CPT)];
    }
    __syncthreads();
  }
}

// ---- D-step -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float caae_log_sigmoid(float y) { return fminf(y, 0.f) - log1pf(expf(-fabsf(y))); }

struct CaaeDP {
  const int* tu;                 // [cnt] user, positive item, negative item of every triple of the slice
  const int* ti;
  const int* tj;
  int cnt, k, ldk;
  float* P;                      // [U, ldk]
  float* Q;                      // [N, ldk]
  float* b;                      // [N]
  float* Pg;                     // [cnt, ldk] the rows as the step found them
  float* Qi;
  float* Qj;
  float* coef;                   // [cnt] c_t
  float* lt;                     // [cnt] -log sigmoid(x_t)
  float* rt;                     // [cnt] |P_u|^2 + |Q_i|^2 + |Q_j|^2 + b_i^2 + b_j^2
  float* bg;                     // [2 cnt] b_i then b_j as the step found them
  int* first;                    // [U + N] the first reference of every row of P, then of Q, in this slice; 0x7f7f7f7f between steps
  int U;
  float lr, beta;
};

constexpr int CAAE_WALK = 8;      // chunks of 64 references in flight per wave of caae_d_update_kernel

// one wave per triple
__global__ __launch_bounds__(256) void caae_d_coef_kernel(const CaaeDP p) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= p.cnt) return;
  const int u = p.tu[t], i = p.ti[t], j = p.tj[t];
  const float* __restrict__ pu = p.P + (size_t)u * p.ldk;
  const float* __restrict__ qi = p.Q + (size_t)i * p.ldk;
  const float* __restrict__ qj = p.Q + (size_t)j * p.ldk;
  float dot = 0.f, sq = 0.f;
  for (int d = lane; d < p.k; d += 64) {
    const float a = pu[d], x = qi[d], y = qj[d];
    p.Pg[(size_t)t * p.ldk + d] = a;
    p.Qi[(size_t)t * p.ldk + d] = x;
    p.Qj[(size_t)t * p.ldk + d] = y;
    dot += a * (x - y);
    sq += (a * a + x * x) + y * y;
  }
  dot = wave_sum(dot);
  sq = wave_sum(sq);
  if (lane == 0) {
    const float bi = p.b[i], bj = p.b[j];
    const float x = dot + (bi - bj);
    const float ls = caae_log_sigmoid(x);
    p.coef[t] = -expf(caae_log_sigmoid(-x)) / (float)p.cnt;      // 1 - sigmoid(x) = sigmoid(-x), without the cancellation
    p.bg[t] = bi;
    p.bg[p.cnt + t] = bj;
    // a minimum does not depend on the order of its updates: integer atomics keep the step reproducible
    atomicMin(&p.first[u], t);
    atomicMin(&p.first[p.U + i], t);
    atomicMin(&p.first[p.U + j], p.cnt + t);
    p.lt[t] = -ls;
    p.rt[t] = sq + (bi * bi + bj * bj);
  }
}

// Wave w < cnt stands for the user of triple w, wave cnt + v (v < 2 cnt) for item reference v of the list [positives | negatives].  The
// wave of a row's FIRST reference (CaaeDP::first, formed by caae_d_coef_kernel) owns the row: it walks the whole list in ascending
// order, adds every reference's contribution, stores the updated row and puts the row's word of `first` back to 0x7f7f7f7f for the
// next step; every other wave leaves at once (whatever it reads there, the owner's index or that filler, is not its own index).
__global__ __launch_bounds__(256) void caae_d_update_kernel(const CaaeDP p) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int cnt = p.cnt;
  if (w >= 3 * cnt) return;
  const bool user = w < cnt;
  const int self = user ? w : w - cnt;                      // index into the list of cnt (users) or 2 cnt (items) references
  const int nref = user ? cnt : 2 * cnt;
  const int row = user ? p.tu[self] : (self < cnt ? p.ti[self] : p.tj[self - cnt]);
  int* own = p.first + (user ? row : p.U + row);
  if (__atomic_load_n(own, __ATOMIC_RELAXED) != self) return;
  constexpr int MAXQ = 4;                                   // k <= 256: at most four factors per lane
  float acc[MAXQ] = {0.f, 0.f, 0.f, 0.f}, pre[MAXQ] = {0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f, bpre = 0.f;
  float* __restrict__ dst = (user ? p.P : p.Q) + (size_t)row * p.ldk;
  {
    const float* __restrict__ g = user ? p.Pg + (size_t)self * p.ldk
                                       : (self < cnt ? p.Qi + (size_t)self * p.ldk : p.Qj + (size_t)(self - cnt) * p.ldk);
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) { const int d = lane + 64 * q; if (d < p.k) pre[q] = g[d]; }
    if (!user) bpre = p.bg[self];
  }
  // the walk: CAAE_WALK chunks of 64 references are loaded before the first is looked at, so a round trip to memory is paid once per
  // 64 * CAAE_WALK references; the chunks are then taken in ascending order
  for (int s0 = 0; s0 < nref; s0 += 64 * CAAE_WALK) {
    int other[CAAE_WALK];
#pragma unroll
    for (int q = 0; q < CAAE_WALK; ++q) {
      const int s = s0 + 64 * q + lane;
      other[q] = -1;
      if (s < nref) other[q] = user ? p.tu[s] : (s < cnt ? p.ti[s] : p.tj[s - cnt]);
    }
#pragma unroll
    for (int q = 0; q < CAAE_WALK; ++q) {
      const int c0 = s0 + 64 * q;
      unsigned long long hits = __ballot(other[q] == row);
      while (hits) {
        const int bit = __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const int ref = c0 + bit;
        const int t = ref < cnt ? ref : ref - cnt;            // the triple of the reference
        const float c = p.coef[t];
        if (user) {
#pragma unroll
          for (int d4 = 0; d4 < MAXQ; ++d4) {
            const int d = lane + 64 * d4;
            if (d < p.k) acc[d4] += c * (p.Qi[(size_t)t * p.ldk + d] - p.Qj[(size_t)t * p.ldk + d]) + p.beta * pre[d4];
          }
        } else {
          const float sc = ref < cnt ? c : -c;
#pragma unroll
          for (int d4 = 0; d4 < MAXQ; ++d4) {
            const int d = lane + 64 * d4;
            if (d < p.k) acc[d4] += sc * p.Pg[(size_t)t * p.ldk + d] + p.beta * pre[d4];
          }
          bacc += sc + p.beta * bpre;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) { const int d = lane + 64 * q; if (d < p.k) dst[d] = pre[q] - p.lr * acc[q]; }
  if (!user && lane == 0) p.b[row] = bpre - p.lr * bacc;
  if (lane == 0) __atomic_store_n(own, 0x7f7f7f7f, __ATOMIC_RELAXED);
}

// ---- reward -----------------------------------------------------------------------------------------------------------------------
// one wave per draw: reward[b, s] = log sigmoid(sign * (<P_u, Q_j> + b_j - 1)), sign = +1 for G, -1 for G'
__global__ __launch_bounds__(256) void caae_reward_kernel(const int* __restrict__ users, const int* __restrict__ items, int nb, int n_s,
                                                          const float* __restrict__ P, const float* __restrict__ Q,
                                                          const float* __restrict__ bq, int k, int ldk, float sign,
                                                          float* __restrict__ reward) {
  const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= (long long)nb * n_s) return;
  const int u = users[t / n_s], j = items[t];
  const float* __restrict__ pu = P + (size_t)u * ldk;
  const float* __restrict__ qj = Q + (size_t)j * ldk;
  float dot = 0.f;
  for (int d = lane; d < k; d += 64) dot += pu[d] * qj[d];
  dot = wave_sum(dot);
  if (lane == 0) reward[t] = caae_log_sigmoid(sign * ((dot + bq[j]) - 1.0f));
}

// ---- policy rows --------------------------------------------------------------------------------------------------------------------
struct CaaePolP {
  const float* R;                // [nb, ld] the generator's sigmoid outputs r
  const float* C;                // [nb, ld] the profiles x
  const unsigned* nu;            // [nb, words] or nullptr (G': no auto-encoder term)
  const int* items;              // [nb, n_s]
  const float* reward;           // [nb, n_s]
  const float* lse;              // [nb] log sum exp(r)
  float* dz;                     // [nb, ld] d loss / d (pre-activation of the output layer)
  float* la;                     // [nb] sum_s log softmax(r)[j_s] * R_s
  float* ae;                     // [nb] sum_k ((r_k - x_k) e_k)^2
  int ld, ncols, words, n_s;
  float pc;                      // lmbda / (nb n_s)  (G': 1 / (nb n_s))
  float ac;                      // 1 - lmbda         (G': 0)
};

constexpr int CAAE_POL_DRAWS = 2048;      // draws of a row staged in LDS; a longer list is read from memory

__global__ __launch_bounds__(256) void caae_policy_kernel(const CaaePolP p) {
  __shared__ int sh_it[CAAE_POL_DRAWS];
  __shared__ float sh_rw[CAAE_POL_DRAWS];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, N = p.ncols, n_s = p.n_s;
  const float* __restrict__ r = p.R + (size_t)b * p.ld;
  const float* __restrict__ x = p.C + (size_t)b * p.ld;
  const unsigned* __restrict__ nu = p.nu ? p.nu + (size_t)b * p.words : nullptr;
  const int* it = p.items + (size_t)b * n_s;
  const float* rw = p.reward + (size_t)b * n_s;
  const float lse = p.lse[b];
  float sr = 0.f, pl = 0.f;
  for (int s = tid; s < n_s; s += 256) {
    const float w = rw[s];
    sr += w;
    pl += (r[it[s]] - lse) * w;
  }
  const float sumR = cfgan_block_sum(sr, red);
  pl = cfgan_block_sum(pl, red);
  if (n_s <= CAAE_POL_DRAWS) {
    for (int s = tid; s < n_s; s += 256) { sh_it[s] = it[s]; sh_rw[s] = rw[s]; }
    __syncthreads();
    it = sh_it;
    rw = sh_rw;
  }
  float* __restrict__ dz = p.dz + (size_t)b * p.ld;
  float aes = 0.f;
  for (int j = tid; j < N; j += 256) {
    float hit = 0.f;
    for (int s = 0; s < n_s; ++s) hit += it[s] == j ? rw[s] : 0.f;      // the row's draws of column j, in draw order
    const float rv = r[j], xv = x[j];
    float dr = -p.pc * (hit - sumR * expf(rv - lse));
    if (p.ac != 0.f) {
      const float e = xv + (nu ? (float)((nu[j >> 5] >> (j & 31)) & 1u) : 0.f);
      const float d = (rv - xv) * e;
      aes += d * d;
      dr += 2.0f * p.ac * d * e;
    }
    dz[j] = dr * (rv * (1.0f - rv));
  }
  aes = cfgan_block_sum(aes, red);
  if (tid == 0) { p.la[b] = pl; p.ae[b] = aes; }
}

// *out = -pc * sum la + ac * sum ae + beta / 2 * sum sq    (sq may be nullptr); one workgroup
__global__ __launch_bounds__(256) void caae_g_loss_kernel(const float* __restrict__ la, const float* __restrict__ ae, int nb, float pc,
                                                          float ac, const float* __restrict__ sq, int nsq, float beta,
                                                          float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f, e = 0.f, q = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) { a += la[i]; e += ae[i]; }
  if (sq) for (int i = threadIdx.x; i < nsq; i += 256) q += sq[i];
  a = cfgan_block_sum(a, red);
  e = cfgan_block_sum(e, red);
  q = cfgan_block_sum(q, red);
  if (threadIdx.x == 0) {
    float l = -pc * a;
    if (ac != 0.f) l += ac * e;
    if (sq) l += beta * (0.5f * q);
    *out = l;
  }
}

// theta -= lr * (g + beta * theta) over n4 float4 slots (pad elements: g = theta = 0 stays 0)
__global__ __launch_bounds__(256) void caae_sgd_kernel(float* __restrict__ th, const float* __restrict__ g, long long n4, float lr,
                                                       float beta) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 t = reinterpret_cast<float4*>(th)[i];
    const float4 d = reinterpret_cast<const float4*>(g)[i];
    t.x -= lr * (d.x + beta * t.x);
    t.y -= lr * (d.y + beta * t.y);
    t.z -= lr * (d.z + beta * t.z);
    t.w -= lr * (d.w + beta * t.w);
    reinterpret_cast<float4*>(th)[i] = t;
  }
}

}  // namespace ganmf
