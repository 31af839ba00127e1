// abi_misc.inc -- C ABI: snapshot / restore, stream timer, profiler, stand-alone GEMM entry
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
int ganmf_snapshot_best(ganmf_handle* h) {
  if (!h) return fail(-1, "null handle");
  TRY(needs_tensors(h, "ganmf_snapshot_best"));
  HIP_TRY(hipSetDevice(h->dev));
  for (Tensor* t : all_tensors(h))
    HIP_TRY(hipMemcpyAsync(t->best, t->p, t->padded() * sizeof(float), hipMemcpyDeviceToDevice, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}

int ganmf_restore_best(ganmf_handle* h) {
  if (!h) return fail(-1, "null handle");
  TRY(needs_tensors(h, "ganmf_restore_best"));
  HIP_TRY(hipSetDevice(h->dev));
  ++h->param_version;
  for (Tensor* t : all_tensors(h))
    HIP_TRY(hipMemcpyAsync(t->p, t->best, t->padded() * sizeof(float), hipMemcpyDeviceToDevice, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}

int ganmf_stream_timer(ganmf_handle* h, int stop, double* ms) {
  if (!h) return fail(-1, "null handle");
  HIP_TRY(hipSetDevice(h->dev));
  if (!h->ev_t0) { HIP_TRY(hipEventCreate(&h->ev_t0)); HIP_TRY(hipEventCreate(&h->ev_t1)); }
  if (!stop) { HIP_TRY(hipEventRecord(h->ev_t0, h->st)); return 0; }
  if (!ms) return fail(-1, "ganmf_stream_timer: null result pointer");
  HIP_TRY(hipEventRecord(h->ev_t1, h->st));
  HIP_TRY(hipEventSynchronize(h->ev_t1));
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, h->ev_t0, h->ev_t1));
  *ms = (double)f;
  return 0;
}

int ganmf_profile_enable(ganmf_handle* h, int on) {
  if (!h) return fail(-1, "null handle");
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  for (auto& r : h->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  h->recs.clear();
  h->prof = on != 0;
  return 0;
}

int ganmf_profile_read(ganmf_handle* h, ganmf_prof_entry* out, int32_t cap, int32_t* n_out) {
  if (!h || !out || !n_out) return fail(-1, "null argument");
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  std::vector<ganmf_prof_entry> acc(T_COUNT);
  for (int i = 0; i < T_COUNT; ++i) {
    memset(&acc[i], 0, sizeof acc[i]);
    snprintf(acc[i].name, sizeof acc[i].name, "%s", kTagName[i]);
  }
  for (auto& r : h->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    acc[r.tag].launches += 1; acc[r.tag].ms += ms; acc[r.tag].flops += r.flops; acc[r.tag].bytes += r.bytes;
  }
  int n = 0;
  for (int i = 0; i < T_COUNT && n < cap; ++i)
    if (acc[i].launches) out[n++] = acc[i];
  *n_out = n;
  return 0;
}

// ganmf_gemm_f32 / ganmf_gemm_f32_ex.  `a_gather` (M ids into the a_rows rows of a K-contiguous A), `bk` (GemmPlan::bk: 32 = the 4-wave staged
// kernel's 32-deep K-tile) and `adam_m` (the fused-Adam epilogue on theta = m = v = 0, lr_t = 1e-3, no L2 term: C returns theta, adam_m the first
// moment, which is (1 - beta1) x the product) reach what the step's launches use and the plain entry cannot ask for.
static int gemm_f32_entry(int device, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K,
                          int a_kmajor, int b_kmajor, int tile, int nsplit, int iters, float* ms,
                          const int32_t* a_gather, int64_t a_rows, int bk, float* adam_m) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1) return fail(-1, "ganmf_gemm_f32: bad argument");
  if (a_gather && (a_kmajor || a_rows < 1)) return fail(-1, "ganmf_gemm_f32_ex: a row list needs a K-contiguous A with a_rows >= 1 rows");
  if (bk != 0 && bk != 32) return fail(-1, "ganmf_gemm_f32_ex: bk must be 0 or 32");
  if (adam_m && (iters > 1 || ms)) return fail(-1, "ganmf_gemm_f32_ex: the Adam epilogue updates its state: one launch, no timing (iters = 1, ms = NULL)");
  if (a_gather)
    for (int64_t r = 0; r < M; ++r)
      if (a_gather[r] < 0 || a_gather[r] >= a_rows) return fail(-1, "ganmf_gemm_f32_ex: row id out of range");
  if (a_kmajor && !b_kmajor) return fail(-1, "ganmf_gemm_f32: the TT layout is not part of the GANMF path");
  if (tile != 0 && tile != 64 && tile != 128) return fail(-1, "ganmf_gemm_f32: tile must be 0, 64 or 128");
  HIP_TRY(hipSetDevice(device));
  const int ar = a_kmajor ? K : (a_gather ? (int)a_rows : M), ac = a_kmajor ? M : K;
  const int br = b_kmajor ? K : N, bc = b_kmajor ? N : K;
  const int lda = round_up(ac, LD_ALIGN), ldb = round_up(bc, LD_ALIGN), ldc = round_up((int)N, LD_ALIGN);
  DevBuf<float> dA, dB, dC, slab, zp, dMom, dAlpha;      // (freed on every return)
  DevBuf<int> dIds;
  TRY(zp.alloc(2048 + 64, true));
  TRY(dA.alloc((size_t)ar * lda, true)); TRY(dB.alloc((size_t)br * ldb, true)); TRY(dC.alloc((size_t)M * ldc, true));
  HIP_TRY(hipMemcpy2D(dA, (size_t)lda * 4, A, (size_t)ac * 4, (size_t)ac * 4, ar, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(dB, (size_t)ldb * 4, B, (size_t)bc * 4, (size_t)bc * 4, br, hipMemcpyHostToDevice));
  GemmP g{};
  g.A = dA; g.lda = lda; g.B = dB; g.ldb = ldb; g.C = dC; g.ldc = ldc;
  g.M = (int)M; g.N = (int)N; g.K = (int)K; g.nbatch = 1; g.epi.kind = EPI_STORE; g.zero_page = zp; g.c_pad_writable = 1;
  if (a_gather) {
    TRY(dIds.alloc((size_t)M, true));
    HIP_TRY(hipMemcpy(dIds, a_gather, (size_t)M * 4, hipMemcpyHostToDevice));
    g.a_gather = dIds;
  }
  if (adam_m) {      // theta (= C), m, v start at zero (the allocation clears)
    const float alpha = 1e-3f;
    TRY(dMom.alloc(2 * (size_t)M * ldc, true)); TRY(dAlpha.alloc(64, true));
    HIP_TRY(hipMemcpy(dAlpha, &alpha, 4, hipMemcpyHostToDevice));
    g.epi.kind = EPI_ADAM; g.epi.adam_theta = dC; g.epi.adam_m = dMom; g.epi.adam_v = dMom + (size_t)M * ldc;
    g.epi.adam_alpha = dAlpha; g.epi.adam_reg = 0.f;
  }
  GemmTune tune;
  tune.tile = tile; tune.nsplit = adam_m ? 1 : nsplit; tune.bk = bk;
  tune.mode = env_mfma_mode(MFMA_DEFAULT);
  tune.ring = tune_env_int("ring", 0);
  if (tune.ring != 0 && tune.ring != 2 && tune.ring != 3 && tune.ring != 4) tune.ring = 0;
  tune.persist = tune_env_int("persist", -1);
  if (tune.persist > 1) tune.persist = 1;
  tune.kg = tune_env_int("kg", 0);
  tune.tile_order = tune_env_int("tile_order", 0);
  if (tune.kg != 0 && tune.kg != 1 && tune.kg != 2 && tune.kg != 4) tune.kg = 0;
  GemmPlan pl = gemm_plan(g.M, g.N, g.K, 1, false, tune, adam_m != nullptr);
  pl.persist = gemm_persist_eligible(g, a_kmajor, b_kmajor, pl, tune.persist) ? 1 : 0;
  if (tune_env_int("skinny", 1) && tile == 0 && nsplit == 0) { if (!plan_skinny(pl, g, a_kmajor != 0) && tune_env_int("skinny_n", 1)) plan_skinny_n(pl, g, a_kmajor != 0); }
  if (env_int("GANMF_X3KG", 0) && pl.mode == MFMA_F32 && pl.tile == 64 && pl.kg == 4 && pl.ring == 3 && !pl.persist) pl.mode = MFMA_BF16X3;      // (tests: the 16-wave split-bf16 kernel)
  if (tune_env_int("bf16w", 0) && tile == 0 && nsplit == 0) plan_bf16w(pl, g, a_kmajor != 0, b_kmajor != 0, tune_env_int("bf16w", 0) >= 2);      // (tests: 2 = wherever eligible)
  if (env_int("GANMF_DEBUG_PLAN", 0))      // (tests assert on the kernel the planner picked, not only on the numbers it produced)
    fprintf(stderr, "[ganmf plan] %-28s M=%d N=%d K=%d batch=1 -> tile %d ring %d kg %d nsplit %d (kps %d) mfma %s wgs %d est %.1f us%s\n", "ganmf_gemm_f32",
            g.M, g.N, g.K, pl.tile, pl.ring, pl.kg, pl.nsplit, pl.kps,
            pl.mode == MFMA_BF16X3 ? "bf16x3" : pl.mode == MFMA_BF16 ? "bf16" : pl.mode == MFMA_F16 ? "f16" : "f32", pl.tiles_m * pl.tiles_n * pl.nsplit, pl.est_us,
            pl.skinny ? " (skinny-K stream)" : pl.skinny_n ? " (skinny-N stream)" : pl.wide32 ? " (64 x 32 tiles, 128-deep K-tiles)" : pl.persist ? " (persistent tile walk)" : "");
  // (the row list is read by the 16-wave kernels' operand fetch only: any other plan would silently multiply the ungathered rows)
  if (a_gather && !(pl.tile == 64 && pl.kg == 4 && !pl.persist && !pl.skinny && !pl.skinny_n && !pl.wide32))
    return fail(-1, "ganmf_gemm_f32_ex: a row list needs a 16-wave 64 x 64 plan (tile = 64, GANMF_TUNE kg=4,ring=3)");
  const size_t slab_elems = gemm_slab_elems(pl, g.M, ldc, 1);
  if (slab_elems) TRY(slab.alloc(slab_elems, true));
  hipStream_t st = nullptr;
  HIP_TRY(gemm_run(st, g, a_kmajor, b_kmajor, pl, slab, slab_elems));
  HIP_TRY(hipDeviceSynchronize());
  if (iters > 1 || ms) {
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    hipEventRecord(a, st);
    for (int i = 0; i < std::max(iters, 1); ++i) gemm_run(st, g, a_kmajor, b_kmajor, pl, slab, slab_elems);
    hipEventRecord(b, st);
    hipEventSynchronize(b);
    float t = 0.f;
    hipEventElapsedTime(&t, a, b);
    if (ms) *ms = t / std::max(iters, 1);
    hipEventDestroy(a); hipEventDestroy(b);
  }
  HIP_TRY(hipMemcpy2D(C, (size_t)N * 4, dC, (size_t)ldc * 4, (size_t)N * 4, M, hipMemcpyDeviceToHost));
  if (adam_m) HIP_TRY(hipMemcpy2D(adam_m, (size_t)N * 4, dMom, (size_t)ldc * 4, (size_t)N * 4, M, hipMemcpyDeviceToHost));
  return 0;
}

int ganmf_gemm_f32(int device, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K,
                   int a_kmajor, int b_kmajor, int tile, int nsplit, int iters, float* ms) {
  return gemm_f32_entry(device, A, B, C, M, N, K, a_kmajor, b_kmajor, tile, nsplit, iters, ms, nullptr, 0, 0, nullptr);
}

int ganmf_gemm_f32_ex(int device, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K,
                      int a_kmajor, int b_kmajor, int tile, int nsplit, int iters, float* ms,
                      const int32_t* a_gather, int64_t a_rows, int bk, float* adam_m) {
  return gemm_f32_entry(device, A, B, C, M, N, K, a_kmajor, b_kmajor, tile, nsplit, iters, ms, a_gather, a_rows, bk, adam_m);
}

