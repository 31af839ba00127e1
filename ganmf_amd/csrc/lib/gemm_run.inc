// gemm_run.inc -- one logical GEMM of the step: plan, launch, split-K reduce (run_gemm)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

int ensure_slab(ganmf_handle* h, size_t elems, int lane) {
  DevBuf<float>& slab = lane ? h->slab2 : h->slab;
  if (elems <= slab.cap) return 0;
  HIP_TRY(hipStreamSynchronize(h->st2));
  return slab.grow(h->st, elems + elems / 4 + 1024, true);
}

// One logical GEMM of the step: plan (tile / ring / split-K), launch, and when split the reduce
// kernel that applies the epilogue.  *sq_count = partial sums per batch written to epi.sq_partials.
// `defer` (plain-store GEMMs only): a split product is left as its slabs for the CONSUMER kernel to sum in split order
// (one launch less); the slabs live in the second workspace so that the GEMMs in between may use the first.
struct SlabRef { const float* p; int nsplit; long long split_stride; };

// `defer_red`: a split product is launched WITHOUT its reduce kernel; the RedP that finishes it (slab sum + epilogue) is
// handed back (part != nullptr) for the caller to attach to a later launch.  `attach`: such a RedP of ANOTHER product, run
// as extra blocks of this GEMM's launch when the plan allows (gemm_bf16s_red), else as its own kernel first.
// The plan of one logical GEMM: the cost model's choice (or `force`) and the arithmetic rewrites of the handle.
GemmPlan plan_gemm(const ganmf_handle* h, int tag_gemm, const GemmP& g, bool akm, bool bkm, const GemmTune* force) {
  const GemmTune& tn = force ? *force : h->tune;
  GemmPlan pl = gemm_plan(g.M, g.N, g.K, std::max(g.nbatch, 1), g.epi.sq_partials != nullptr, tn, g.epi.kind == EPI_ADAM);
  pl.persist = gemm_persist_eligible(g, akm, bkm, pl, tn.persist) ? 1 : 0;
  // a plan for the 16-wave fp32 ring kernel (one 64 x 64 tile per CU) runs the 16-wave split-bf16 loop instead: same grid, same split,
  // same epilogue, 6 / 16 of the MFMA cycles (gemm_bf16k.hpp)
  // (only under MFMA_AUTO: a handle created with GANMF_FLAG_MFMA_F32 / mfma="f32" runs the fp32 MFMA everywhere, as documented)
  if (!force && h->tune.mode == MFMA_AUTO && pl.mode == MFMA_F32 && pl.tile == 64 && pl.kg == 4 && pl.ring == 3 && !pl.persist && !(akm && !bkm) &&
      (tag_gemm != T_GEMM_GUB || h->gub_x3) && tag_gemm != T_GEMM_GV &&      // (gUb / gV: their other form is the fp32 pair_kernel -- unless gV runs staged)
      (((h->x3kg & 1) && !akm && !bkm) || ((h->x3kg & 2) && bkm))) pl.mode = MFMA_BF16X3;      // bit 0: NT products, bit 1: products with a K-major B
  // ... and a single-piece (bf16 / fp16) plan with a CU per workgroup takes the same 16-wave kernel in its one-piece form (bit 2)
  if (!force && (h->x3kg & 4) && (pl.mode == MFMA_F16 || pl.mode == MFMA_BF16) && pl.tile == 64 && pl.ring == 3 && pl.bk != 32 && !pl.persist &&
      !(akm && !bkm)) pl.kg = 4;
  // K <= 64 behind a wide output: the product is a stream (gemm_skinny.hpp)
  if (!force && h->skinny) { if (!plan_skinny(pl, g, akm) && h->skinny_n) plan_skinny_n(pl, g, akm); }
  // two K slices per 64 x 64 tile where 64 x 32 tiles fill the chip unsplit (gemm_bf16w.hpp)
  if (!force && h->bf16w) plan_bf16w(pl, g, akm, bkm, h->bf16w >= 2);
  return pl;
}

// `plan`: run exactly this plan (stage_pass: the plan of ONE minibatch's product, replayed over the batches of a pass).
int run_gemm(ganmf_handle* h, int tag_gemm, int tag_red, GemmP g, bool akm, bool bkm, int* sq_count = nullptr,
             double extra_bytes = 0, int lane = 0, const GemmTune* force = nullptr, SlabRef* defer = nullptr,
             RedP* defer_red = nullptr, const RedP* attach = nullptr, const GemmPlan* plan = nullptr) {
  if (g.nbatch < 1) g.nbatch = 1;
  g.zero_page = h->zero_page;
  if (g.epi.kind == EPI_ADAM) g.n_fastest = 1;      // (every fused-Adam product, not only the paired launch)
  hipStream_t st = lane ? h->st2 : h->st;
  GemmPlan pl = plan ? *plan : plan_gemm(h, tag_gemm, g, akm, bkm, force);
  if (defer) *defer = SlabRef{g.C, 1, 0};
  // (a deep split behind a small output is summed 16 threads per element by the reduce kernel: not left to the consumer)
  const bool deferred = defer && pl.nsplit > 1 && g.epi.kind == EPI_STORE && g.nbatch == 1 &&
                        reduce_groups((long long)g.M * ((g.N + 3) >> 2), pl.nsplit) == 1;
  const int slab_lane = deferred ? 1 : lane;
  const bool lent = slab_lane && h->slab2_lent;      // (gen_update's lazy pass: a block of the pass arena stands in for slab2)
  if (pl.nsplit > 1 && !lent) TRY(ensure_slab(h, gemm_slab_elems(pl, g.M, g.ldc, g.nbatch), slab_lane));
  float* slab = lent ? h->slab2_lent : slab_lane ? h->slab2.get() : h->slab.get();
  const size_t slab_elems = lent ? h->slab2_lent_elems : slab_lane ? h->slab2.cap : h->slab.cap;
  const bool wants_sq = g.epi.sq_partials != nullptr;
  const int nredg = GEMM_RED_GRID;      // blocks (and partials) of a stand-alone slab sum
  const int sqc = !wants_sq ? 0 : (pl.nsplit > 1 ? nredg : pl.sq_count);
  if (sq_count) *sq_count = sqc;
  if (h->debug_plan) {
    const long long key = ((long long)tag_gemm << 48) ^ ((long long)g.M << 32) ^ ((long long)g.N << 16) ^ g.K;
    if (std::find(h->seen_plans.begin(), h->seen_plans.end(), key) == h->seen_plans.end()) {
      h->seen_plans.push_back(key);
      fprintf(stderr, "[ganmf plan] %-28s M=%d N=%d K=%d batch=%d -> tile %d ring %d kg %d nsplit %d (kps %d) mfma %s wgs %d est %.1f us%s\n",
              kTagName[tag_gemm], g.M, g.N, g.K, g.nbatch, pl.tile, pl.ring, pl.kg, pl.nsplit, pl.kps,
              pl.mode == MFMA_BF16X3 ? "bf16x3" : pl.mode == MFMA_BF16 ? "bf16" : pl.mode == MFMA_F16 ? "f16" : "f32",
              pl.tiles_m * pl.tiles_n * pl.nsplit * g.nbatch, pl.est_us,
              pl.skinny ? " (skinny-K stream)" : pl.skinny_n ? " (skinny-N stream)" : pl.wide32 ? " (64 x 32 tiles, 128-deep K-tiles)" : pl.persist ? " (persistent tile walk)" : "");
    }
  }
  const double fl = g.nbatch * gemm_flops(g.M, g.N, g.K), by = gemm_bytes((double)g.nbatch * g.M, g.N, g.K) + extra_bytes;
  if (defer_red) defer_red->part = nullptr;
  if (attach && attach->part) {
    const int n4 = (attach->N + 3) / 4;
    const int nred = (int)std::min<long long>(GEMM_RED_GRID, ((long long)attach->M * n4 + 255) / 256);
    const bool combined = pl.mode == MFMA_BF16X3 && pl.tile == 64 && pl.bk == 32 && pl.nsplit == 1 && akm && bkm &&
                          !pl.persist && g.nbatch == 1 && attach->epi.sq_partials == nullptr;
    if (combined) {
      Scope s(h, T_GWD_RED, fl, by + 4.0 * (attach->nsplit + 1) * attach->M * attach->N, st);
      GemmP q = g;
      fill_plan(q, pl);
      const int ng = pl.tiles_m * pl.tiles_n;
      GANMF_LAUNCH(gemm_bf16s_red, dim3(ng + nred), dim3(256), 0, st, q, *attach, nred);
      HIP_TRY(hipGetLastError());
      return 0;
    }
    {
      Scope s(h, tag_red, 0, 4.0 * (attach->nsplit + 1) * attach->M * attach->N, st);
      RedP r = *attach;
      GANMF_LAUNCH(splitk_reduce_kernel, dim3(GEMM_RED_GRID, 1), dim3(256), 0, st, r);
      HIP_TRY(hipGetLastError());
    }
  }
  if (defer_red && pl.nsplit > 1 && !deferred && g.nbatch == 1) {    // GEMM now, its reduce rides in a later launch
    Scope s(h, tag_gemm, fl, by, st);
    GemmP q = g;
    fill_plan(q, pl);
    q.C = slab; q.c_split_stride = (long long)g.M * g.ldc; q.c_batch_stride = (long long)g.M * g.ldc;
    HIP_TRY(gemm_dispatch(st, q, akm, bkm, pl));
    RedP r{};
    r.part = slab; r.nsplit = pl.nsplit; r.out = g.C; r.ld = g.ldc; r.M = g.M; r.N = g.N;
    r.batch_stride = g.c_batch_stride; r.epi = g.epi; r.epi.sq_stride = nredg;
    r.split_stride = (long long)g.M * g.ldc;
    *defer_red = r;
    if (sq_count && wants_sq) *sq_count = nredg;
    return 0;
  }
  if (deferred) {     // slabs only: the consumer sums them
    Scope s(h, tag_gemm, fl, by + 4.0 * pl.nsplit * g.M * g.N, st);
    GemmP q = g;
    q.tiles_m = pl.tiles_m; q.tiles_n = pl.tiles_n; q.nsplit = pl.nsplit; q.k_per_split = pl.kps;
    q.C = slab; q.c_split_stride = (long long)g.M * g.ldc; q.c_batch_stride = (long long)g.M * g.ldc;
    HIP_TRY(gemm_dispatch(st, q, akm, bkm, pl));
    *defer = SlabRef{slab, pl.nsplit, (long long)g.M * g.ldc};
    return 0;
  }
  if (!h->prof || pl.nsplit == 1) {
    Scope s(h, tag_gemm, fl, by + (pl.nsplit > 1 ? 8.0 * pl.nsplit * g.nbatch * g.M * g.N : 0), st);
    HIP_TRY(gemm_run(st, g, akm, bkm, pl, slab, slab_elems, nredg));
    return 0;
  }
  {  // profiled, separate reduce kernel: bracket the GEMM and the reduce separately
    Scope s(h, tag_gemm, fl, by, st);
    GemmP q = g;
    q.tiles_m = pl.tiles_m; q.tiles_n = pl.tiles_n; q.nsplit = pl.nsplit; q.k_per_split = pl.kps;
    q.C = slab; q.c_split_stride = (long long)g.nbatch * g.M * g.ldc; q.c_batch_stride = (long long)g.M * g.ldc;
    hipError_t e;
    e = gemm_dispatch(st, q, akm, bkm, pl);
    HIP_TRY(e);
  }
  {
    Scope s(h, tag_red, 0, 4.0 * (pl.nsplit + 1) * g.nbatch * g.M * g.N, st);
    RedP r{};
    r.part = slab; r.nsplit = pl.nsplit; r.out = g.C; r.ld = g.ldc; r.M = g.M; r.N = g.N;
    r.batch_stride = g.c_batch_stride; r.epi = g.epi; r.epi.sq_stride = nredg;
    r.split_stride = (long long)g.nbatch * g.M * g.ldc;
    GANMF_LAUNCH(splitk_reduce_kernel, dim3(nredg, g.nbatch), dim3(256), 0, st, r);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// Early touch of the Adam streams of a fused-Adam product with an [M, ld] parameter (GemmP::adam_touch): only while the three arrays fit half of the
// chip's 8 x 4 MiB of L2 -- the touched lines must still be there when the row pass asks for them, and the operands stream through the same caches.
// Measured: 11 MB (V at ML-1M) pays, 88 MB (Wd + We) costs 10 us of a 44 us launch (profiles/r09_wgrad_touch.md); nothing in between has been run.
inline int adam_touch_for(const ganmf_handle* h, long long M, long long ld) { return h->adam_touch && 12 * M * ld <= (16ll << 20) ? 1 : 0; }

// the combined launches (front_kernel, de_dcoef_kernel) carry the 16-wave split-bf16 loop where the stand-alone product would run it:
// GANMF_X3KG bit 0, and only when the handle leaves the arithmetic to the planner (a forced fp32-MFMA handle keeps the fp32 MFMA)
inline bool combined_x3(const ganmf_handle* h) { return (h->x3kg & 1) != 0 && h->tune.mode == MFMA_AUTO; }

