// fp32 GEMM on the bf16 matrix cores, operands split ONCE when they are staged (gfx950 / CDNA4).
//
// Same contract as gemm_f32_mfma (GemmP, operand layouts NT / NN / TN, zero-page convention, split-K slabs,
// shared epilogue) with a different K loop:
//   * every fp32 operand element is split exactly into three bf16 pieces x = hi + mid + lo (gemm_f32.hpp,
//     split_bf16x3: round-to-nearest at each level) by the thread that LOADS it, and the pieces are written to
//     three LDS planes per operand; a.b is accumulated in fp32 from the six piece products of weight >= 2^-18
//     on v_mfma_f32_32x32x16_bf16.
//     (Splitting at fragment-read time instead — fp32 tiles in LDS, each wave splitting what it reads — repeats the
//     VALU work in both waves that share a fragment; hipcc emits VALU work and MFMAs in blocks, whose issue times
//     add on a SIMD (tools/ubench/mfma_valu.hip), and that variant was 3 % slower at 4096^3 and 30 % slower in
//     bf16 mode.)
//   * HBM/L2 -> registers -> split -> LDS.  One LDS buffer, the next K-tile prefetched into registers while the
//     current one is multiplied; two workgroups per CU cover each other's barriers.
//   * LDS plane layouts (dword = two bf16 with consecutive k, low half first):
//       K-contiguous operand  [row][BK/2], the 16-byte chunk (8 k's) index XOR-swizzled by the row
//                             -> one conflict-free ds_read_b128 per piece and fragment;
//       K-major operand       (round 5) [k][R] bf16 -- the operand's own orientation, two rows per dword -- with the 16-byte chunk
//                             (8 rows) index XORed by f(k & 3), read with the TRANSPOSING ds_read_b64_tr_b16: two reads per
//                             piece and fragment (k + 0..3 and k + 4..7 of the lane's eight) at 256 B/clk instead of four
//                             ds_read_b32 at 128 B/clk (rounds 1-4: [k/2][R] dwords of (k, k + 1) pairs), conflict-free; an item
//                             is four consecutive rows of TWO k-rows (two 16-byte loads whose lanes tile whole 256-byte row
//                             segments: a first version with 8 rows of one k-row per item -- 16-byte loads at a 32-byte lane
//                             stride -- tripled the time the NN kernels wait for memory), paired ALONG the row like a
//                             K-contiguous item and filed as two 8-byte stores per piece.
//     A lane (i = lane & 31, h = lane >> 5) holds k = 16c + 8h + 0..7 of MFMA step c for both operands.
//   * NPIECE = 1 rounds each operand to a single bf16 (RNE), or with F16 = true to a single fp16 after an exact
//     power-of-two scale and a clamp to the fp16 range: the mixed-precision modes (MFMA_BF16 / MFMA_F16).
#pragma once
#include "gemm_f32.hpp"

namespace ganmf {

// LDS byte addresses.  A K loop converts its shared-memory pointer ONCE (the conversion from a generic pointer carries a null check: a
// compare and a select) and forms every plane address in front of the loop as an integer; piece, plane and buffer are compile-time
// constants added to it, which the ds instructions take as their immediate offset.
__device__ inline unsigned lds_addr(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)      // (LDS pointers are 32 bits wide in the device pass only)
  return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p;
#else
  (void)p;
  return 0u;
#endif
}
// A base address the compiler cannot take apart again.  The workgroup's LDS starts at a known address, so hipcc re-associates base + constant
// sums and pushes ALL constants into the instruction's offset -- and those that exceed its 16 bits (the second plane buffer of the 16-wave loops:
// + 48 KiB and more) come back as one v_add_u32 per access.  A loop keeps one such base per plane buffer and operand; what it adds to it fits.
// (OPAQUE = false: the plain sum -- the one-piece loops' planes all lie below 64 KiB)
template <bool OPAQUE = true>
__device__ inline unsigned lds_base(unsigned addr) {
  if constexpr (OPAQUE) asm("" : "+v"(addr));
  return addr;
}
template <class T>
__device__ inline T lds_read(unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(__attribute__((address_space(3))) const T*)addr;
#else
  (void)addr;
  return T{};
#endif
}
template <class T>
__device__ inline void lds_write(unsigned addr, const T v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(__attribute__((address_space(3))) T*)addr = v;
#else
  (void)addr; (void)v;
#endif
}

template <int R, int BK, bool KM>
struct SplitStage {
  static constexpr int NW = R * BK / 8;       // work items (8 elements each) per K-tile
  static constexpr int NI = NW / 256;         // per thread
  static constexpr int PLANE = R * BK / 2;    // dwords per piece plane
  static constexpr int CH = BK / 8;           // K-contiguous: 16-byte chunks per row
  static constexpr int RQ = R / 4;            // K-major: row quads per k-row
  static constexpr int KROW = R / 2;          // K-major: dwords per k-row of a plane
  static_assert(R == 64 || R == 128, "K-major chunk swizzle is laid out for 64- and 128-row operand tiles");
  // K-major: XOR on the chunk index of k-row k.  A transposing read covers k-rows k0 .. k0 + 3 (k0 a multiple of four) x 16 rows per
  // 16-lane group, two groups per 32-lane half: with 128-byte k-rows (R = 64) rows k0 + 2, k0 + 3 fall on the banks of k0, k0 + 1 and
  // move to the other half of their 128 bytes; with 256-byte k-rows (R = 128) all four share their banks and take four different
  // 64-byte groups (SQ_LDS_BANK_CONFLICT 0)
  __device__ static inline int swzk(int k) { return R == 64 ? ((k & 3) >> 1) << 2 : (k & 3) << 2; }
  static_assert(NW % 256 == 0 && NI >= 1, "tile too small for 256 threads");
  static_assert(BK == 32 || BK == 64, "BK must be 32 or 64");

  __device__ static inline int swz(int row) { return BK == 32 ? (row >> 2) & 3 : (row >> 1) & 7; }

  const float* zp;          // this lane's 32-byte line of the zero page
  const float* ptr[NI];     // source of the next tile (KM: first of the two k-rows; a lane whose columns lie past ld: its zero-page line)
  int aux[NI];              // !KM: pointer increment per tile (0: zero-page lane); KM: first k-row of the item
  long long kinc[NI];       // K-major: floats per K-tile (0: zero-page lane)
  int krow[NI];             // K-major: floats from the item's first k-row to its second (ld; 0: zero-page lane)
  unsigned dst[NI];         // LDS byte address in piece plane 0 (K-major: of the item's first k-row)
  unsigned dst1[NI];        // K-major: of its second k-row

  // `lds_planes`: LDS byte address of this operand's piece plane 0 (lds_addr)
  __device__ inline void init(const float* __restrict__ base, int ld, int r0, int rlimit, int kbeg,
                              const float* zero, int tid, unsigned lds_planes) {
    zp = zero + (tid & 255) * 8;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int w = j * 256 + tid;
      if constexpr (!KM) {
        const int row = w / CH, c8 = w % CH;
        const bool ok = (r0 + row) < rlimit;
        ptr[j] = ok ? base + (size_t)(r0 + row) * ld + kbeg + 8 * c8 : zp;
        aux[j] = ok ? BK : 0;
        dst[j] = lds_planes + 4u * (unsigned)(row * (BK / 2) + 4 * (c8 ^ swz(row)));
      } else {
        const int kp = w / RQ, rq = w % RQ;
        const bool ok = (r0 + 4 * rq) < ld;
        ptr[j] = ok ? base + (size_t)(kbeg + 2 * kp) * ld + r0 + 4 * rq : zp;
        kinc[j] = ok ? (long long)BK * ld : 0;
        krow[j] = ok ? ld : 0;
        aux[j] = 2 * kp;
        dst[j] = lds_planes + 4u * (unsigned)((2 * kp) * KROW + 4 * ((rq >> 1) ^ swzk(2 * kp)) + 2 * (rq & 1));
        dst1[j] = lds_planes + 4u * (unsigned)((2 * kp + 1) * KROW + 4 * ((rq >> 1) ^ swzk(2 * kp + 1)) + 2 * (rq & 1));
      }
    }
  }

  // fetch this thread's share of the tile that starts kleft k's before the end of the K range
  __device__ inline void load(float4 (&v)[NI][2], int kleft) {
    const float* s0[NI];
    const float* s1[NI];
    const float* const z = zp;      // (read in front of the branch below)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      s0[j] = ptr[j];
      if constexpr (!KM) { s1[j] = ptr[j] + 4; ptr[j] += aux[j]; }
      else { s1[j] = ptr[j] + krow[j]; ptr[j] += kinc[j]; }
    }
    if constexpr (KM) {
      // only the LAST K-tile of a slice can be partial: its missing k-rows come from the zero page.  A scalar branch (kleft is uniform),
      // so that every other tile executes no compare and no select for its addresses; the empty asm keeps hipcc from turning the branch
      // back into selects
      if (kleft < BK) {
        asm volatile("; partial last K-tile");
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          s0[j] = aux[j] < kleft ? s0[j] : z;
          s1[j] = aux[j] + 1 < kleft ? s1[j] : z;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      v[j][0] = *reinterpret_cast<const float4*>(s0[j]);
      v[j][1] = *reinterpret_cast<const float4*>(s1[j]);
    }
  }

  // split / round and write the pieces to this operand's planes of the buffer `buf_bytes` behind the one init() was given
  // (piece q at + q * PLANE dwords: buffer and piece are constants of the instruction)
  template <int NPIECE, bool F16 = false>
  __device__ inline void store(const float4 (&v)[NI][2], float scale = 1.f, unsigned buf_bytes = 0u) const {
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      // the four pairs of this item: 8 consecutive k of one row, or 8 consecutive rows of one k-row
      // (no private arrays here: hipcc parks them in scratch / LDS)
      const float4 a = v[j][0], b = v[j][1];
      u32x4 pc[3];
      auto one = [&](float x0, float x1, auto qq) {
        constexpr int q = decltype(qq)::value;
        if constexpr (NPIECE == 3) {
          unsigned h, m, l;
          split_bf16x3(x0, x1, h, m, l);
          pc[0][q] = h; pc[1][q] = m; pc[2][q] = l;
        } else if constexpr (F16) {
          pc[0][q] = cvt_pk_f16(x0 * scale, x1 * scale);
        } else {
          pc[0][q] = cvt_pk_bf16(x0, x1);
        }
      };
      // (either layout pairs along its dwords: eight k of one row; or four rows of k-row k, then four rows of k-row k + 1)
      one(a.x, a.y, std::integral_constant<int, 0>{}); one(a.z, a.w, std::integral_constant<int, 1>{});
      one(b.x, b.y, std::integral_constant<int, 2>{}); one(b.z, b.w, std::integral_constant<int, 3>{});
#pragma unroll
      for (int q = 0; q < NPIECE; ++q) {
        if constexpr (KM) {
          typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
          lds_write<u32x2>(dst[j] + buf_bytes + 4u * (unsigned)(q * PLANE), u32x2{pc[q][0], pc[q][1]});
          lds_write<u32x2>(dst1[j] + buf_bytes + 4u * (unsigned)(q * PLANE), u32x2{pc[q][2], pc[q][3]});
        } else {
          lds_write<u32x4>(dst[j] + buf_bytes + 4u * (unsigned)(q * PLANE), pc[q]);
        }
      }
    }
  }

  // The fragment reads with the lane's address formed ONCE: frag_off() is the byte offset inside a piece plane of the 32-row block at
  // tile row rb, MFMA step c, lane (i, h) -- what frag() below computes per call -- and frag_at() reads one piece at an LDS byte address
  // (plane base + frag_off + constants).  A further MFMA step is + frag_step bytes in the K-major image (c stands outside its chunk XOR).
  static constexpr unsigned frag_step = 16 * KROW * 4;
  __device__ static inline unsigned frag_off(int rb, int c, int i, int h) {
    if constexpr (!KM) {
      return 4u * (unsigned)((rb + i) * (BK / 2) + 4 * ((2 * c + h) ^ swz(i)));
    } else {
      const int l16 = i & 15, gi = i >> 4, qq = l16 >> 2, pp = l16 & 3;
      return (unsigned)((16 * c + 8 * h + qq) * (KROW * 4) + ((((rb >> 3) + 2 * gi + (pp >> 1)) ^ swzk(qq)) << 4) + ((pp & 1) << 3));
    }
  }
  __device__ static inline u32x4 frag_at(unsigned addr) {
    if constexpr (!KM) {
      return lds_read<u32x4>(addr);
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
      typedef __attribute__((address_space(3))) s16x4* lds_s16x4_p;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)addr);
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(addr + 4 * (KROW * 4)));
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#else
      (void)addr;
      return u32x4{0u, 0u, 0u, 0u};
#endif
    }
  }

  // one piece of the fragment of the 32-row block at tile row rb, MFMA step c, lane (i, h)
  __device__ static inline u32x4 frag(const unsigned* __restrict__ plane, int rb, int c, int i, int h) {
    if constexpr (!KM) {
      return *reinterpret_cast<const u32x4*>(plane + (rb + i) * (BK / 2) + 4 * ((2 * c + h) ^ swz(i)));
    } else {
      // ds_read_b64_tr_b16: lane 4 qq + pp of a 16-lane group supplies the address of k-row qq, rows 4 pp .. 4 pp + 3 of a 4 (k) x 16 (rows)
      // block and receives row (lane & 15) of the four k-rows.  Group gi = (i >> 4) takes rows 16 gi .. 16 gi + 15 of the 32-row block;
      // lane half h the k-rows 16 c + 8 h + 0..7, in two reads (+ 0..3, + 4..7: the same k & 3, hence the same chunk XOR).
      const int l16 = i & 15, gi = i >> 4, qq = l16 >> 2, pp = l16 & 3;
      const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned*)plane;
      const unsigned addr = base + (unsigned)((16 * c + 8 * h + qq) * (KROW * 4) + ((((rb >> 3) + 2 * gi + (pp >> 1)) ^ swzk(qq)) << 4) + ((pp & 1) << 3));
#if defined(__HIP_DEVICE_COMPILE__)      // (LDS pointers are 32 bits wide in the device pass only)
      typedef __attribute__((address_space(3))) s16x4* lds_s16x4_p;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)addr);
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(addr + 4 * (KROW * 4)));
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#else
      (void)addr;
      return u32x4{0u, 0u, 0u, 0u};
#endif
    }
  }
};

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int BM, int BN, int BK, int NPIECE>
struct Bf16sLds {      // floats of LDS one workgroup needs: the piece planes, or the C tile the epilogue stages there
  static constexpr int OPER = NPIECE * (BM * BK / 2 + BN * BK / 2);
  static constexpr int DW = OPER > BM * BN ? OPER : BM * BN;
};

// (body = device function of (block index, blocks of this GEMM): one launch can carry more than one piece of work,
// gemm_multi.hpp; `smem` is the launch's only LDS object, Bf16sLds<...>::DW floats)
// GRAM: the symmetric product of gram_stats.hpp, as in gemm_f32_body
// ROWSQ: the decode product of disc_rows.hpp -- the same K loop behind rowsq_epilogue (per-row sums of squared residuals, nothing stored)
template <int BM, int BN, int BK, bool AKM, bool BKM, int NPIECE, bool F16 = false, bool GRAM = false, bool ROWSQ = false>
__device__ __forceinline__ void gemm_bf16s_body(const GemmP& p, const int bid, const int nblk, float* __restrict__ smem) {
  static_assert(!F16 || NPIECE == 1, "fp16 pieces only in the single-piece (mixed precision) mode");
  const float sa = (F16 && p.a_scale != 0.f) ? p.a_scale : 1.f, sb = (F16 && p.b_scale != 0.f) ? p.b_scale : 1.f;
  using SA = SplitStage<BM, BK, AKM>;
  using SB = SplitStage<BN, BK, BKM>;
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int NC = BK / 16;
  static_assert(NPIECE == 1 || NPIECE == 3, "pieces per operand");
  static_assert(BM % 32 == 0 && BN % 32 == 0, "row XOR of the K-major layout needs 32-row blocks");
  static_assert(Bf16sLds<BM, BN, BK, NPIECE>::OPER == NPIECE * (SA::PLANE + SB::PLANE), "LDS budget");
  unsigned* const planes_a = reinterpret_cast<unsigned*>(smem);
  unsigned* const planes_b = planes_a + NPIECE * SA::PLANE;
  const unsigned lds_a = lds_addr(smem), lds_b = lds_a + 4u * (unsigned)(NPIECE * SA::PLANE);      // (the one conversion of this launch's LDS pointer)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  int tm, tn, sp = 0, bz = 0;
  if constexpr (GRAM) gram_tile_coords(p, bid, nblk, tm, tn);
  else tile_coords(p, bid, nblk, tm, tn, sp, bz);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = sp * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  const int nt = (kend - kbeg + BK - 1) / BK;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  SA la;
  SB lb;
  la.init(p.A + (size_t)bz * p.a_batch_stride, p.lda, m0, p.M, kbeg, p.zero_page, tid, lds_a);
  lb.init(p.B, p.ldb, n0, p.N, kbeg, p.zero_page, tid, lds_b);

  float4 ra[SA::NI][2], rb[SB::NI][2];
  int kleft = kend - kbeg;
  la.load(ra, kleft);
  lb.load(rb, kleft);
  kleft -= BK;
  la.template store<NPIECE, F16>(ra, sa);
  lb.template store<NPIECE, F16>(rb, sb);
  __syncthreads();

  // K-major fragments: this lane's address in piece plane 0 of every 32-row block, formed once (MFMA step and piece are constants of the read)
  unsigned fa[TM], fb[TN];
#pragma unroll
  for (int a = 0; a < TM; ++a) fa[a] = lds_a + SA::frag_off(wr * WM + a * 32, 0, li, lh);
#pragma unroll
  for (int b = 0; b < TN; ++b) fb[b] = lds_b + SB::frag_off(wc * WN + b * 32, 0, li, lh);

  u32x4 pa[2][TM][NPIECE], pb[2][TN][NPIECE];
  auto load_frags = [&](int set, int c) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int q = 0; q < NPIECE; ++q) {
        if constexpr (AKM) pa[set][a][q] = SA::frag_at(fa[a] + c * SA::frag_step + 4u * (unsigned)(q * SA::PLANE));
        else pa[set][a][q] = SA::frag(planes_a + q * SA::PLANE, wr * WM + a * 32, c, li, lh);
      }
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int q = 0; q < NPIECE; ++q) {
        if constexpr (BKM) pb[set][b][q] = SB::frag_at(fb[b] + c * SB::frag_step + 4u * (unsigned)(q * SB::PLANE));
        else pb[set][b][q] = SB::frag(planes_b + q * SB::PLANE, wc * WN + b * 32, c, li, lh);
      }
  };
  // Two accumulators per block in the split mode: the hi.hi products (weight 1) go to `acc`, the five correction
  // products (weights 2^-9 .. 2^-18) to `accl`, which stays ~2^-8 of `acc`, so the small terms are not rounded away
  // against a large running sum; the two are added once, before the epilogue.  With one accumulator the path missed
  // the two tightest Adam-amplified parity checks (5.6e-5 / 6.7e-5 against a 5e-5 bound the fp32 MFMA meets); with
  // two, every GEMM of the step can run on it and the whole GPU suite passes.  __launch_bounds__(256, 2) keeps the
  // 128 accumulator registers of the 128x128 tile within two workgroups per CU.
  f32x16 accl[NPIECE == 3 ? TM : 1][NPIECE == 3 ? TN : 1];
  if constexpr (NPIECE == 3) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) accl[a][b][r] = 0.f;
  }
  auto mfmas = [&](int set) {
    // piece products in increasing weight, blocks innermost (dependent MFMAs are TM*TN issues apart)
    constexpr int NT = NPIECE == 3 ? 6 : 1;
    constexpr int ta[6] = {1, 0, 2, 1, 0, 0}, tb[6] = {1, 2, 0, 0, 1, 0};   // (mid,mid) (hi,lo) (lo,hi) (mid,hi) (hi,mid) (hi,hi)
#pragma unroll
    for (int t6 = 0; t6 < NT; ++t6)
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
          const int ia = NT == 6 ? ta[t6] : 0, ib = NT == 6 ? tb[t6] : 0;
          if (NT == 6 && t6 < 5)
            accl[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[set][a][ia]),
                                                                 __builtin_bit_cast(bf16x8, pb[set][b][ib]), accl[a][b], 0, 0, 0);
          else if constexpr (F16)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, pa[set][a][ia]),
                                                               __builtin_bit_cast(f16x8, pb[set][b][ib]), acc[a][b], 0, 0, 0);
          else
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[set][a][ia]),
                                                                __builtin_bit_cast(bf16x8, pb[set][b][ib]), acc[a][b], 0, 0, 0);
        }
  };

  for (int it = 0; it < nt; ++it) {
    const bool more = it + 1 < nt;
    if (more) {                      // next K-tile into registers while this one is multiplied
      la.load(ra, kleft);
      lb.load(rb, kleft);
      kleft -= BK;
    }
    load_frags(0, 0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c + 1 < NC) load_frags((c + 1) & 1, c + 1);
      mfmas(c & 1);
    }
    __syncthreads();                 // every wave has read its fragments: the planes may be overwritten
    if (more) {
      la.template store<NPIECE, F16>(ra, sa);
      lb.template store<NPIECE, F16>(rb, sb);
      __syncthreads();
    }
  }
  if constexpr (NPIECE == 3) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b) acc[a][b] += accl[a][b];
  }
  if constexpr (F16) {
    if (sa != 1.f || sb != 1.f) {      // undo the operand scaling in fp32 (powers of two: exact)
      const float un = 1.f / (sa * sb);
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) acc[a][b] *= un;
    }
  }
  if constexpr (GRAM) {
    static_assert(NPIECE == 3 && !F16 && !AKM && !BKM, "the symmetric product is an NT product in the exact three-way split");
    gram_epilogue<BM, BN, TM, TN>(p, acc, smem, TileCoord{tm, tn, sp, bz, m0, n0});
  } else if constexpr (ROWSQ) {
    static_assert(NPIECE == 3 && !F16, "the per-row residual sums are formed in the exact three-way split");
    rowsq_epilogue<BM, BN, TM, TN>(p, acc, smem, TileCoord{tm, tn, sp, bz, m0, n0});
  } else
  gemm_epilogue<BM, BN, TM, TN, 1, AKM && BKM>(p, acc, smem, TileCoord{tm, tn, sp, bz, m0, n0});
}

template <int BM, int BN, int BK, bool AKM, bool BKM, int NPIECE, bool F16 = false>
__global__ __launch_bounds__(256, 2) void gemm_bf16s_mfma(const GemmP p) {
  __shared__ __attribute__((aligned(16))) float smem[Bf16sLds<BM, BN, BK, NPIECE>::DW];
  gemm_bf16s_body<BM, BN, BK, AKM, BKM, NPIECE, F16>(p, (int)blockIdx.x, (int)gridDim.x, smem);
}

template <int BM, int BN, int BK, int NPIECE, bool F16 = false>
inline hipError_t gemm_bf16s_launch(hipStream_t st, const GemmP& p, bool akm, bool bkm) {
  const int grid = p.tiles_m * p.tiles_n * p.nsplit * p.nbatch;
  if (grid <= 0) return hipSuccess;
  if (!akm && !bkm) GANMF_LAUNCH((gemm_bf16s_mfma<BM, BN, BK, false, false, NPIECE, F16>), dim3(grid), dim3(256), 0, st, p);
  else if (!akm && bkm) GANMF_LAUNCH((gemm_bf16s_mfma<BM, BN, BK, false, true, NPIECE, F16>), dim3(grid), dim3(256), 0, st, p);
  else if (akm && bkm) GANMF_LAUNCH((gemm_bf16s_mfma<BM, BN, BK, true, true, NPIECE, F16>), dim3(grid), dim3(256), 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

template <int NPIECE, bool F16>
inline hipError_t gemm_bf16k_launch(hipStream_t st, const GemmP& p, bool akm, bool bkm);      // gemm_bf16k.hpp: the 16-wave form

inline hipError_t gemm_dispatch_staged(hipStream_t st, const GemmP& p, bool akm, bool bkm, const GemmPlan& pl) {
  if (pl.tile == 64 && pl.kg == 4) {
    if (pl.mode == MFMA_BF16X3) return gemm_bf16k_launch<3, false>(st, p, akm, bkm);
    if (pl.mode == MFMA_F16) return gemm_bf16k_launch<1, true>(st, p, akm, bkm);
    if (pl.mode == MFMA_BF16) return gemm_bf16k_launch<1, false>(st, p, akm, bkm);
  }
  if (pl.mode == MFMA_F16)
    return pl.tile == 128 ? gemm_bf16s_launch<128, 128, 32, 1, true>(st, p, akm, bkm) : gemm_bf16s_launch<64, 64, 64, 1, true>(st, p, akm, bkm);
  if (pl.mode == MFMA_BF16X3 && pl.tile == 64 && pl.bk == 32) return gemm_bf16s_launch<64, 64, 32, 3>(st, p, akm, bkm);
  if (pl.mode == MFMA_BF16X3)
    return pl.tile == 128 ? gemm_bf16s_launch<128, 128, 32, 3>(st, p, akm, bkm) : gemm_bf16s_launch<64, 64, 64, 3>(st, p, akm, bkm);
  return pl.tile == 128 ? gemm_bf16s_launch<128, 128, 32, 1>(st, p, akm, bkm) : gemm_bf16s_launch<64, 64, 64, 1>(st, p, akm, bkm);
}

}  // namespace ganmf
