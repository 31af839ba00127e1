// als_rows.hpp -- one half sweep of implicit-feedback ALS (WRMF), the per-row part: for every row u of a confidence matrix with at
// least one stored entry, with P(u) its stored columns and c its confidences,
//     B = G + sum_{j in P(u)} (c_j - 1) y_j y_j^T + reg I,    b = sum_{j in P(u)} c_j y_j,    X[u, :] = B^-1 b
// (MatrixFactorization/IALSRecommender.py:137-201, _run_epoch / _update_row of the reference, which inverts B with np.linalg.inv;
// G = Y^T Y is formed once per half sweep by the library's TN product).  Rows without a stored entry are not touched.
//
// als_rows_mfma_kernel (32 < k <= 256): one workgroup of four waves per row.  The profile's factor rows go through LDS in tiles of
//   ALS_GATHER entries; the rank-|P(u)| update is a symmetric product over the lower-triangle pairs of 32 x 32 tiles, each pair owned by
//   one wave and accumulated in registers on v_mfma_f32_32x32x2_f32 (fp32 operands: A = (c - 1) y, B = y).  When the profile is
//   through, G and reg I are added and B's lower triangle is stored PACKED in LDS over the gather tile (131 584 B at k = 256), factored
//   in place as L L^T in panels of 32 columns -- diagonal block in the registers of one wave, panel solve one thread per row, trailing
//   update over all threads: three barriers per panel -- and the two substitutions run panel by panel the same way.
// als_rows_small_kernel (k <= 32): one wave per row, four rows per workgroup, everything on the VALU: lane r keeps row r of B in
//   registers, the factorisation is the diagonal-block routine of the large kernel.
// Every sum runs in a fixed order and nothing is shared between rows: the same bytes on every call.  A pivot that is not positive
// (reg <= 0 with a rank-deficient Y, or a reg below the rounding of G with one) leaves the row's factors as they were and raises
// bad[1 + u] and bad[0] with plain stores; the host names the first such row.
#pragma once
#include <hip/hip_runtime.h>

namespace ganmf {

constexpr int ALS_MAX_K = 256;
constexpr int ALS_GATHER = 32;      // profile entries per gather tile (sixteen K = 2 MFMA steps)
constexpr int ALS_THREADS = 256;

struct AlsP {
  const float* Y;            // factors of the side held fixed, [n_cols, ldy], pad columns zero
  const float* G;            // Y^T Y, [k, ldg]
  float* X;                  // factors of the side being solved, [n_rows, ldx]
  int ldy, ldg, ldx;
  const long long* indptr;   // confidence matrix of this side: CSR over n_rows
  const int* indices;
  const float* conf;
  int n_rows, k;
  float reg;
  int* bad;                  // [1 + n_rows], zero at launch: bad[0] any row failed, bad[1 + u] row u failed
};

__device__ inline int als_tri(int r) { return r * (r + 1) / 2; }

// L L^T of a 32 x 32 block in the registers of one wave: lane r (and r + 32) holds row r, a[c] = B[r][c] for c <= r (entries above the
// diagonal are never read by another lane).  Rows at and past `nb` must be rows of the identity.  Fixed order; *bad is wave-uniform.
__device__ inline void als_chol32(float (&a)[32], int r, int nb, bool* bad) {
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    float d = __shfl(a[j], j);
    if (j < nb && !(d > 0.f)) { *bad = true; d = 1.f; }
    const float s = sqrtf(d);
    const float l = r == j ? s : a[j] / s;
    a[j] = l;
#pragma unroll
    for (int c = j + 1; c < 32; ++c) a[c] -= l * __shfl(l, c);
  }
}

// forward substitution with the diagonal block at (J, J) of the packed triangle Ls: lane r holds b[J + r], returns z[J + r]
__device__ inline float als_fwd32(const float* Ls, int J, int nb, int r, float v) {
  for (int j = 0; j < nb; ++j) {
    const float zj = __shfl(v, j) / Ls[als_tri(J + j) + J + j];
    if (r == j) v = zj;
    else if (r > j && r < nb) v -= Ls[als_tri(J + r) + J + j] * zj;
  }
  return v;
}

// backward substitution with the transpose of the same block: lane c holds z[J + c], returns x[J + c]
__device__ inline float als_bwd32(const float* Ls, int J, int nb, int c, float v) {
  for (int j = nb - 1; j >= 0; --j) {
    const float xj = __shfl(v, j) / Ls[als_tri(J + j) + J + j];
    if (c == j) v = xj;
    else if (c < j) v -= Ls[als_tri(J + j) + J + c] * xj;
  }
  return v;
}

// dynamic LDS of the large kernel in floats: the gather tile [ALS_GATHER][kp] with its two weight vectors, later the packed triangle
// with b / z and the failure word behind it
inline size_t als_lds_floats(int k) {
  const size_t kp = (size_t)(k + 31) / 32 * 32;
  const size_t gather = (size_t)ALS_GATHER * kp + 2 * ALS_GATHER;
  const size_t tri = ((size_t)k * (k + 1) / 2 + 3) / 4 * 4 + 2 * ALS_MAX_K + 4;
  return gather > tri ? gather : tri;
}

template <int MAXP>      // tile pairs per wave: ceil(nt (nt + 1) / 2 / 4) at most
__global__ __launch_bounds__(ALS_THREADS) void als_rows_mfma_kernel(AlsP p) {
  extern __shared__ float als_lds[];
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const long long beg = p.indptr[u];
  const int cnt = (int)(p.indptr[u + 1] - beg);
  if (cnt == 0) return;      // (the whole workgroup: no barrier has been reached)
  const int k = p.k, nt = (k + 31) / 32, kp = nt * 32, kp4 = kp / 4, npairs = nt * (nt + 1) / 2;
  float* const Ys = als_lds;                          // [ALS_GATHER][kp]
  float* const ws = als_lds + ALS_GATHER * kp;        // c - 1 per entry of the tile
  float* const cs = ws + ALS_GATHER;                  // c
  f32x16 acc[MAXP];
  int ti[MAXP], tj[MAXP];
#pragma unroll
  for (int s = 0; s < MAXP; ++s) {
    for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
    const int pr = wave + 4 * s;
    int t = 0;
    while ((t + 1) * (t + 2) / 2 <= pr) ++t;
    ti[s] = pr < npairs ? t : -1;
    tj[s] = pr - t * (t + 1) / 2;
  }
  float bacc = 0.f;      // thread c < kp: b[c]
  for (int base = 0; base < cnt; base += ALS_GATHER) {
    __syncthreads();      // the tile before this one has been consumed
    const int left = cnt - base;
    if (tid < ALS_GATHER) {
      const float c = tid < left ? p.conf[beg + base + tid] : 0.f;
      ws[tid] = tid < left ? c - 1.f : 0.f;
      cs[tid] = c;
    }
    for (int i = tid; i < ALS_GATHER * kp4; i += ALS_THREADS) {
      const int e = i / kp4, c4 = i - e * kp4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < left) v = *reinterpret_cast<const float4*>(p.Y + (size_t)p.indices[beg + base + e] * p.ldy + 4 * c4);
      *reinterpret_cast<float4*>(Ys + e * kp + 4 * c4) = v;
    }
    __syncthreads();
    if (tid < kp)
      for (int e = 0; e < ALS_GATHER; ++e) bacc += cs[e] * Ys[e * kp + tid];
    const int steps = left >= ALS_GATHER ? ALS_GATHER / 2 : (left + 1) / 2;      // (entries past the profile's end are zero rows)
#pragma unroll
    for (int s = 0; s < MAXP; ++s) {
      if (ti[s] < 0) continue;
      const float* ya = Ys + 32 * ti[s] + li;
      const float* yb = Ys + 32 * tj[s] + li;
      for (int kk = 0; kk < steps; ++kk) {
        const int e = 2 * kk + lh;
        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[e] * ya[e * kp], yb[e * kp], acc[s], 0, 0, 0);
      }
    }
  }
  __syncthreads();      // the gather tile is dead: the packed triangle takes its place
  float* const Ls = als_lds;
  float* const bs = als_lds + (k * (k + 1) / 2 + 3) / 4 * 4;      // b, later x
  float* const zs = bs + ALS_MAX_K;
  int* const badw = reinterpret_cast<int*>(zs + ALS_MAX_K);
  // C / D layout of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int s = 0; s < MAXP; ++s) {
    if (ti[s] < 0) continue;
    const int col = 32 * tj[s] + li;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * ti[s] + (i & 3) + 8 * (i >> 2) + 4 * lh;
      if (row < k && col <= row) Ls[als_tri(row) + col] = acc[s][i] + p.G[(size_t)row * p.ldg + col] + (row == col ? p.reg : 0.f);
    }
  }
  if (tid < k) bs[tid] = bacc;
  if (tid == 0) *badw = 0;
  __syncthreads();
  // ---- L L^T in place, panels of 32 columns ----
  for (int J = 0; J < k; J += 32) {
    const int nb = k - J < 32 ? k - J : 32;
    if (wave == 0) {      // diagonal block in registers
      float a[32];
#pragma unroll
      for (int c = 0; c < 32; ++c) a[c] = (li < nb && c <= li) ? Ls[als_tri(J + li) + J + c] : (li >= nb && c == li ? 1.f : 0.f);
      bool bad = false;
      als_chol32(a, li, nb, &bad);
      if (lane < nb) {
#pragma unroll
        for (int c = 0; c < 32; ++c)
          if (c <= lane) Ls[als_tri(J + lane) + J + c] = a[c];
      }
      if (bad && lane == 0) *badw = 1;
    }
    __syncthreads();
    for (int r = J + nb + tid; r < k; r += ALS_THREADS) {      // panel: row r of L[., J .. J + nb)
      float* row = Ls + als_tri(r) + J;
      for (int c = 0; c < nb; ++c) {
        const float* lc = Ls + als_tri(J + c) + J;
        float v = row[c];
        for (int t = 0; t < c; ++t) v -= row[t] * lc[t];
        row[c] = v / lc[c];
      }
    }
    __syncthreads();
    for (int r = J + nb + (tid >> 5); r < k; r += ALS_THREADS / 32) {      // trailing update of the lower triangle
      const float* lr = Ls + als_tri(r) + J;
      for (int c = J + nb + (tid & 31); c <= r; c += 32) {
        const float* lc = Ls + als_tri(c) + J;
        float s = 0.f;
        for (int t = 0; t < nb; ++t) s += lr[t] * lc[t];
        Ls[als_tri(r) + c] -= s;
      }
    }
    __syncthreads();
  }
  // ---- L z = b ----
  for (int J = 0; J < k; J += 32) {
    const int nb = k - J < 32 ? k - J : 32;
    if (wave == 0) {
      const float v = als_fwd32(Ls, J, nb, li, li < nb ? bs[J + li] : 0.f);
      if (lane < nb) zs[J + lane] = v;
    }
    __syncthreads();
    for (int r = J + nb + tid; r < k; r += ALS_THREADS) {
      const float* lr = Ls + als_tri(r) + J;
      float s = 0.f;
      for (int t = 0; t < nb; ++t) s += lr[t] * zs[J + t];
      bs[r] -= s;
    }
    __syncthreads();
  }
  // ---- L^T x = z (x over b) ----
  for (int J = (nt - 1) * 32; J >= 0; J -= 32) {
    const int nb = k - J < 32 ? k - J : 32;
    if (wave == 0) {
      const float v = als_bwd32(Ls, J, nb, li, li < nb ? zs[J + li] : 0.f);
      if (lane < nb) bs[J + lane] = v;
    }
    __syncthreads();
    for (int c = tid; c < J; c += ALS_THREADS) {
      float s = 0.f;
      for (int t = 0; t < nb; ++t) s += Ls[als_tri(J + t) + c] * bs[J + t];
      zs[c] -= s;
    }
    __syncthreads();
  }
  if (*badw) {
    if (tid == 0) { p.bad[1 + u] = 1; p.bad[0] = 1; }
  } else if (tid < k) {
    p.X[(size_t)u * p.ldx + tid] = bs[tid];
  }
}

constexpr int ALS_SMALL_WAVE_LDS = ALS_GATHER * 32 + 2 * ALS_GATHER;      // floats per wave: gather tile + weights, later the packed triangle

__global__ __launch_bounds__(ALS_THREADS) void als_rows_small_kernel(AlsP p) {
  __shared__ float lds[4 * ALS_SMALL_WAVE_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int k = p.k;
  const int u0 = blockIdx.x * 4, u = u0 + wave;
  // every wave walks as many tiles as the longest of the workgroup's four rows (the barriers are the workgroup's)
  int maxcnt = 0, cnt = 0;
  long long beg = 0;
  for (int w = 0; w < 4; ++w) {
    if (u0 + w >= p.n_rows) break;
    const long long b0 = p.indptr[u0 + w];
    const int c0 = (int)(p.indptr[u0 + w + 1] - b0);
    if (w == wave) { beg = b0; cnt = c0; }
    maxcnt = c0 > maxcnt ? c0 : maxcnt;
  }
  float* const Yw = lds + wave * ALS_SMALL_WAVE_LDS;      // [ALS_GATHER][32]
  float* const ws = Yw + ALS_GATHER * 32;
  float* const cs = ws + ALS_GATHER;
  float a[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) a[c] = 0.f;
  float bacc = 0.f;
  for (int base = 0; base < maxcnt; base += ALS_GATHER) {
    __syncthreads();
    const int left = cnt - base;      // (<= 0: this wave's row is through; it fills zeros)
    if (lane < ALS_GATHER) {
      const float c = lane < left ? p.conf[beg + base + lane] : 0.f;
      ws[lane] = lane < left ? c - 1.f : 0.f;
      cs[lane] = c;
    }
    for (int i = lane; i < ALS_GATHER * 8; i += 64) {
      const int e = i >> 3, c4 = i & 7;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < left) v = *reinterpret_cast<const float4*>(p.Y + (size_t)p.indices[beg + base + e] * p.ldy + 4 * c4);
      *reinterpret_cast<float4*>(Yw + e * 32 + 4 * c4) = v;
    }
    __syncthreads();
    if (left > 0) {
      for (int e = lh; e < ALS_GATHER; e += 2) {      // the two half waves take the even and the odd entries
        const float yr = Yw[e * 32 + li];
        const float w = ws[e] * yr;
        bacc += cs[e] * yr;
#pragma unroll
        for (int c = 0; c < 32; ++c) a[c] += w * Yw[e * 32 + c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) a[c] += __shfl_xor(a[c], 32);
  bacc += __shfl_xor(bacc, 32);
  const bool active = cnt > 0;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    if (li < k) { if (c <= li) a[c] += p.G[(size_t)li * p.ldg + c] + (c == li ? p.reg : 0.f); }
    else a[c] = c == li ? 1.f : 0.f;
  }
  bool bad = false;
  als_chol32(a, li, k, &bad);
  __syncthreads();      // the gather tiles are dead
  float* const Lw = Yw;
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < 32; ++c)
      if (c <= lane) Lw[als_tri(lane) + c] = a[c];
  }
  __syncthreads();
  float v = als_fwd32(Lw, 0, k, li, li < k ? bacc : 0.f);
  v = als_bwd32(Lw, 0, k, li, v);
  if (!active) return;
  if (bad) {
    if (lane == 0) { p.bad[1 + u] = 1; p.bad[0] = 1; }
  } else if (lane < k) {
    p.X[(size_t)u * p.ldx + lane] = v;
  }
}

}  // namespace ganmf
