// step_ganmf.inc -- GANMF: the discriminator and generator updates (GANMF.py:131-139,175-203)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// CSR row expansion of the real rows (+ ones column, + DisGANMF's float(uid) column), embedding lookup Ub = U[uids] and the
// generator GEMM F = Ub . V^T -> rows [nb, 2nb) of XF (GANMF.py:82-83,183-184).  One launch when the generator GEMM is
// planned onto the 16-wave fp32 ring kernel (front_kernel: the GEMM fetches its A rows from U through the row list, the
// row expansion runs as extra workgroups of the same grid); else the two kernels one after the other.
// The generator product of ONE minibatch of nb rows as the step launches it: *front = it rides in the combined launch with the row
// expansion (front_kernel, rows gathered by the operand fetch); else the plan run_gemm draws for the stand-alone product on Ub.
GemmPlan generator_plan(ganmf_handle* h, int nb, bool* front) {
  const int N = h->N, k = h->k;
  GemmP g{};
  g.A = h->Ub; g.lda = h->ldk; g.B = h->V.p; g.ldb = h->ldk;
  g.C = h->XF + (size_t)nb * h->ldN; g.ldc = h->ldN;
  g.M = nb; g.N = N; g.K = k; g.epi.kind = EPI_STORE; g.nbatch = 1;
  g.zero_page = h->zero_page;
  // K = num_factors is at most four K-tiles: a split would trade three of them for a reduce launch and keep the GEMM out of
  // the combined launch (B = 64 at ML-1M shape: 4.5 + 5.2 + 4.6 us as three kernels, ~8 us as one)
  GemmPlan pl = gemm_plan(g.M, g.N, g.K, 1, false, h->tune, /*no_split=*/(h->multi & 1) != 0 && k <= 256);
  pl.persist = gemm_persist_eligible(g, false, false, pl, h->tune.persist) ? 1 : 0;
  *front = (h->multi & 1) && plan_is_f32_64_kg(pl, 4) && pl.nsplit == 1;
  // a low-precision handle (mfma = "f16" | "bf16"): the stand-alone product would run the 16-wave one-piece loop (plan_gemm, GANMF_X3KG bit 2);
  // the combined launch carries that loop (front_lp_kernel)
  if (!*front && (h->multi & 1) && (h->x3kg & 4) && low_precision(h) && plan_is_lp_64(pl) && pl.nsplit == 1) { pl.kg = 4; *front = true; }
  if (*front) return pl;
  return plan_gemm(h, T_GEMM_GEN, g, false, false, nullptr);
}

// ---- staged discriminator pass ----------------------------------------------------------------------------------------------
// The generator is frozen while the discriminator trains (GANMF.py:176-189: one shuffle, then every minibatch through opt_disc),
// so nothing a discriminator step reads of U, V or the URM depends on the steps before it.  stage_pass therefore expands the CSR rows
// of ALL full minibatches of the call (one launch) and forms all their generated rows (one batched launch: batch i = minibatch i, the
// SAME 64 x 64 tiles, K order and arithmetic as the per-step launch, hence the same bits) into XF_pass -- minibatch i owns rows
// [2iB, 2iB + B) = X, [2iB + B, 2iB + 2B) = F, the [real ; generated] block every consumer of XF already expects -- and the steps of the
// pass run without their row-expansion + generator launch (10.4 of a 131 us step at the ML-1M shape).  A ragged last minibatch keeps the
// per-step launch.  lr_t of the staged steps comes from open_steps_kernel (one launch per pass).
inline int lazy_tab_slot(const ganmf_handle* h, int p);
bool stage_pass_plan(ganmf_handle* h, int64_t nfull, GemmPlan* pl, bool* front) {
  if (!h->pass_stage || nfull < 4 || h->sparse_d || nfull > h->tab_cap) return false;
  *pl = generator_plan(h, h->B, front);
  if (!*front && (pl->persist || pl->nsplit != 1)) return false;      // (only one-launch forms are replayed as batches)
  const size_t need = (size_t)nfull * 2 * h->B * h->ldN;
  if (need > h->XF_pass.cap) {      // grown on demand; never more than a quarter of the free device memory
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    if ((need - h->XF_pass.cap) * sizeof(float) > free_b / 4) return false;
  }
  return true;
}

// The per-pass buffers at the size of a whole epoch (U / B full minibatches), allocated by the FIRST training call of a handle whatever its
// length: a later, longer call then finds them in place (allocation synchronises the device and zeroes the block -- 179 MB at the ML-1M
// shape -- which belongs in a warm-up call, not in the middle of a training run).  Best effort: on failure the calls grow them on demand.
// One chunk of the gUb arena, ZEROED: the GEMM and slab stores mask columns >= k, and adam_rows_flush_kernel reads whole ldk-wide rows
// of every block -- the pad columns k..ldk must be the zeros every other buffer of the library holds there (a recycled allocation
// with a NaN bit pattern in a pad column would reach user_embeddings' pads and from there F = Ub . V^T; tests/test_gpu_multi_launch.py
// poisons the allocator to see this).
static bool lazy_chunk_alloc(ganmf_handle* h, size_t elems) {
  DevBuf<float> chunk;
  if (chunk.alloc(elems, false) != 0) return false;
  if (hipMemsetAsync(chunk, 0, elems * sizeof(float), h->st) != hipSuccess) return false;
  h->lazy_chunks.push_back(std::move(chunk));
  return true;
}
// (best effort = a failure must leave no trace: neither HIP's sticky last-error, which the next launch check of the same call would
// report as its own, nor this thread's message)
struct BestEffort {
  std::string saved;
  BestEffort() : saved(g_err) {}
  ~BestEffort() { (void)hipGetLastError(); g_err = saved; }
};
static bool fits_quarter_of_free(size_t bytes) {
  size_t free_b = 0, total_b = 0;
  return hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes <= free_b / 4;
}
void prealloc_pass_buffers(ganmf_handle* h, bool ragged) {      // (ragged: the owner-split schedule of a sharded fit never stages its discriminator passes)
  if (h->pass_buffers_tried) return;
  h->pass_buffers_tried = true;
  const int64_t nfull = h->U / std::max(h->B, 1);
  if (nfull < 4) return;
  BestEffort guard;
  GemmPlan pl{};
  bool front = false;
  if (!ragged && stage_pass_plan(h, nfull, &pl, &front)) {
    const size_t need = (size_t)nfull * 2 * h->B * h->ldN;
    if (need > h->XF_pass.cap) {
      (void)h->XF_pass.alloc(need, true);
    }
    const size_t need_u = front ? 0 : (size_t)nfull * h->B * h->ldk;
    if (need_u > h->Ub_pass.cap && fits_quarter_of_free((need_u - h->Ub_pass.cap) * sizeof(float))) {
      (void)h->Ub_pass.alloc(need_u, true);
    }
  }
  if (h->lazy_rows && h->cfg.g_reg == 0.f) {
    const size_t need = (size_t)h->U * h->ldk;
    if (need > h->Ub_sched.cap && fits_quarter_of_free((need - h->Ub_sched.cap) * sizeof(float))) {
      (void)h->Ub_sched.alloc(need, true);
    }
    // the arena of a pass's gUb slabs (here: sixteen slabs per step, at most 512 MiB; more is added when a pass needs it) and its tables
    if (h->lazy_chunks.empty()) {
      const size_t want = std::min<size_t>((size_t)128 << 20, std::max<size_t>((size_t)16 << 20, (size_t)(nfull + 1) * 16 * h->B * h->ldk));
      if (fits_quarter_of_free(want * sizeof(float))) lazy_chunk_alloc(h, want);
    }
    const size_t T = (size_t)nfull + 2;
    if (2 * T > h->lazy_stage.cap) (void)h->lazy_stage.alloc(2 * (T + 16), false);
    if (2 * T > h->lazy_tab.cap) (void)h->lazy_tab.alloc(2 * (T + 16), false);
  }
}

// open_g: > 0 = the call's first generator pass updates user_embeddings per pass (lazy_pass_begin): lr_t of its open_g steps is written
// by the same launch that writes the discriminator pass's (block 0 of the row expansion)
// *g_opened: set once the launch that advances the generator's beta powers (open_g > 0) has been issued -- a failure before that point
// (growing XF_pass / Ub_pass) leaves them untouched and the caller's PassGuard must not roll them back to a save that was never written
// gen = false (a call without discriminator passes): the CSR rows only -- the generator pass reads its real rows from the staged blocks
// (ganmf_train_epoch: `x_staged`), no generated rows are formed and no discriminator step is opened
int stage_pass(ganmf_handle* h, const int* rows_dev, int64_t nfull, const GemmPlan& pl0, bool front, int uid_col, int row_offset, int open_g,
               bool* g_opened, bool gen = true) {
  const int N = h->N, k = h->k, B = h->B;
  const size_t need = (size_t)nfull * 2 * B * h->ldN;
  if (need > h->XF_pass.cap) {
    HIP_TRY(hipStreamSynchronize(h->st2));
    TRY(h->XF_pass.grow(h->st, need, true));      // (zeroed: the padding columns of the generated rows are never written)
  }
  const size_t need_u = (front || !gen) ? 0 : (size_t)nfull * B * h->ldk;
  TRY(h->Ub_pass.grow(h->st, need_u, true));
  const int rows = (int)(nfull * B);
  {
    DensP d{h->urm.indptr, h->urm.indices, h->data, rows_dev, rows, N, h->XF_pass, h->ldN, h->Ue.p, h->ldk, (front || !gen) ? nullptr : h->Ub_pass,
            h->scal, 0, 0, 0.f, uid_col, row_offset};
    d.stage_b = B;
    d.open_d_slot = S_TAB; d.open_d_count = gen ? (int)nfull : 0; d.lr_d = h->cfg.d_lr;
    d.open_g_slot = lazy_tab_slot(h, 0); d.open_g_count = open_g; d.lr_g = h->cfg.g_lr;
    d.nseg = std::max(1, std::min(16, (h->ldN + 8191) / 8192));
    Scope s(h, T_DENSIFY, 0, 4.0 * rows * (N + 2 * k));
    GANMF_LAUNCH(densify_rows_kernel, dim3(rows * d.nseg), dim3(256), 0, h->st, d);
    HIP_TRY(hipGetLastError());
    if (open_g > 0 && g_opened) *g_opened = true;
  }
  if (!gen) return 0;
  GemmP g{};
  g.B = h->V.p; g.ldb = h->ldk; g.lda = h->ldk;
  g.C = h->XF_pass + (size_t)B * h->ldN; g.ldc = h->ldN; g.c_batch_stride = (long long)2 * B * h->ldN;
  g.M = B; g.N = N; g.K = k; g.epi.kind = EPI_STORE; g.nbatch = (int)nfull;
  g.zero_page = h->zero_page;
  if (front) {
    g.A = h->Ue.p; g.a_gather = rows_dev; g.a_gather_batch = B;
    GemmPlan pl = pl0;
    if (combined_x3(h)) pl.mode = MFMA_BF16X3;      // what front_kernel<4, true> runs
    fill_plan(g, pl);
    Scope s(h, T_GEMM_GEN, nfull * gemm_flops(g.M, g.N, g.K), gemm_bytes((double)nfull * g.M, g.N, g.K));
    HIP_TRY(gemm_dispatch(h->st, g, false, false, pl));
    return 0;
  }
  g.A = h->Ub_pass; g.a_batch_stride = (long long)B * h->ldk;
  return run_gemm(h, T_GEMM_GEN, T_RED_GEN, g, false, false, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, &pl0);
}

int rows_and_generator(ganmf_handle* h, const int* rows_dev, int nb, int which, int aslot, int uid_col, int row_offset) {
  if (which == 0 && h->front_staged) return 0;      // X, F and lr_t of this step were staged in front of the pass (stage_pass)
  // generator step of a call whose CSR rows were staged (round 6): the reference walks the SAME slices of one shuffle in its discriminator and
  // its generator loop (GANMF.py:175-203), so the real rows of this minibatch -- with their ones / float(uid) columns, for both halves of the
  // block -- are in XF already; only the generated rows are formed.  (Lazy generator pass only: the per-step row expansion also gathers Ub and
  // opens the optimizer step, which a lazy pass has done for all its steps at once.)
  const bool xs = which == 1 && h->x_staged && h->lazy_pass;
  const int N = h->N, k = h->k;
  // generator pass with the per-pass update of U (lazy_pass_begin): Ub already points at this minibatch's embeddings as of this step,
  // lr_t of the step has its table slot
  const bool lazy = which == 1 && h->lazy_pass;
  DensP d{h->urm.indptr, h->urm.indices, h->data, rows_dev, nb, N, h->XF, h->ldN, h->Ue.p, h->ldk, lazy ? nullptr : h->Ub, h->scal, which,
          lazy ? -1 : aslot, which ? h->cfg.g_lr : h->cfg.d_lr, uid_col, row_offset};
  GemmP g{};
  g.A = h->Ub; g.lda = h->ldk; g.B = h->V.p; g.ldb = h->ldk;
  g.C = h->XF + (size_t)nb * h->ldN; g.ldc = h->ldN;
  g.M = nb; g.N = N; g.K = k; g.epi.kind = EPI_STORE; g.nbatch = 1;
  g.zero_page = h->zero_page;
  bool is_front = false;
  GemmPlan pl = generator_plan(h, nb, &is_front);
  if (is_front) {
    if (h->debug_plan) {
      const long long key = ((long long)T_GEMM_GEN << 48) ^ ((long long)g.M << 32) ^ ((long long)g.N << 16) ^ g.K;
      if (std::find(h->seen_plans.begin(), h->seen_plans.end(), key) == h->seen_plans.end()) {
        h->seen_plans.push_back(key);
        fprintf(stderr, "[ganmf plan] %-28s M=%d N=%d K=%d batch=1 -> tile 64 ring 3 kg 4 nsplit 1 (kps %d) mfma %s wgs %d est %.1f us (one launch with the %d CSR rows)\n",
                kTagName[T_GEMM_GEN], g.M, g.N, g.K, pl.kps, pl.mode == MFMA_F16 ? "f16" : pl.mode == MFMA_BF16 ? "bf16" : combined_x3(h) ? "bf16x3" : "f32",
                pl.tiles_m * pl.tiles_n, pl.est_us, nb);
      }
    }
    Scope s(h, T_FRONT, gemm_flops(g.M, g.N, g.K), gemm_bytes(g.M, g.N, g.K) + 4.0 * nb * (N + 2 * k));
    if (!lazy) { g.A = h->Ue.p; g.a_gather = rows_dev; }        // A row r = U[rows[r]]: the lookup rides in the operand fetch
    fill_plan(g, pl);
    const int nrow_blocks = xs ? 0 : nb;      // (staged real rows: the launch is the generator GEMM alone)
    if (pl.mode == MFMA_F16) GANMF_LAUNCH(front_lp_kernel<true>, dim3(pl.tiles_m * pl.tiles_n + nrow_blocks), dim3(1024), 0, h->st, g, d);
    else if (pl.mode == MFMA_BF16) GANMF_LAUNCH(front_lp_kernel<false>, dim3(pl.tiles_m * pl.tiles_n + nrow_blocks), dim3(1024), 0, h->st, g, d);
    else if (combined_x3(h)) GANMF_LAUNCH((front_kernel<4, true>), dim3(pl.tiles_m * pl.tiles_n + nrow_blocks), dim3(1024), 0, h->st, g, d);
    else GANMF_LAUNCH(front_kernel<4>, dim3(pl.tiles_m * pl.tiles_n + nrow_blocks), dim3(1024), 0, h->st, g, d);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (!xs) {
    Scope s(h, T_DENSIFY, 0, 4.0 * nb * (N + 2 * k));
    d.nseg = std::max(1, std::min(16, (h->ldN + 8191) / 8192));      // wide rows (C4: 50 000 columns): several workgroups per row
    GANMF_LAUNCH(densify_rows_kernel, dim3(nb * d.nseg), dim3(256), 0, h->st, d);
    HIP_TRY(hipGetLastError());
  }
  return run_gemm(h, T_GEMM_GEN, T_RED_GEN, g, false, false);
}

// ---- shared front of both steps: X rows (+ones column), Ub, F, E = [X;F|1].We_ext ----------------
int step_front(ganmf_handle* h, const int* rows_dev, int nb, int which) {
  const int N = h->N, k = h->k, e = h->e;
  const int aslot = which ? h->g_alpha : h->d_alpha;
  const bool lazy = which == 1 && h->lazy_pass;
  if ((which == 1 && h->sparse_g) || (which == 0 && h->sparse_d)) {
    // sparse regime: Er from the CSR rows, X never materialised, the encode GEMM runs on the generated half only
    TRY(dp_join(h, PEND_WE));
    {
      Scope s(h, T_DENSIFY, 0, 4.0 * nb * (2 * k + e) + 4.0 * (double)h->urm.nnz / std::max(h->U, 1) * nb * e);
      GANMF_LAUNCH(sparse_front_kernel, dim3(nb), dim3(256), 0, h->st, h->urm.indptr.get(), h->urm.indices.get(), h->data.get(), rows_dev, nb, N,
                         h->XF, h->ldN, h->Ue.p.get(), h->ldk, lazy ? nullptr : h->Ub, h->scal.get(), which, lazy ? -1 : aslot, which ? h->cfg.g_lr : h->cfg.d_lr, h->We.p.get(), h->lde, e, h->E.get());
      HIP_TRY(hipGetLastError());
    }
    {
      GemmP g{};
      g.A = h->Ub; g.lda = h->ldk; g.B = h->V.p; g.ldb = h->ldk;
      g.C = h->XF + (size_t)nb * h->ldN; g.ldc = h->ldN;
      g.M = nb; g.N = N; g.K = k; g.epi.kind = EPI_STORE;
      TRY(run_gemm(h, T_GEMM_GEN, T_RED_GEN, g, false, false));
    }
    {
      TRY(dp_join(h, PEND_WE));
      GemmP g{};
      g.A = h->XF + (size_t)nb * h->ldN; g.lda = h->ldN; g.B = h->We.p; g.ldb = h->lde;
      g.C = h->E + (size_t)nb * h->lde; g.ldc = h->lde; g.M = nb; g.N = e; g.K = N + 1; g.epi.kind = EPI_STORE;
      TRY(run_gemm(h, T_GEMM_ENC, T_RED_ENC, g, false, true));
    }
    return 0;
  }
  TRY(rows_and_generator(h, rows_dev, nb, which, aslot, -1, 0));   // X rows, Ub, F = Ub . V^T -> rows [nb, 2nb) of XF  (GANMF.py:82-83)
  {  // E = [X;F | 1] . We_ext  (bias = row N); the ones column E[:, e] is never overwritten  (GANMF.py:64-65)
    TRY(dp_join(h, PEND_WE));     // (data-parallel: the previous step's encoder update ran on the side lane under densify + generator GEMM)
    GemmP g{};
    g.A = h->XF; g.lda = h->ldN; g.B = h->We.p; g.ldb = h->lde;
    g.C = h->E; g.ldc = h->lde; g.M = 2 * nb; g.N = e; g.K = N + 1; g.epi.kind = EPI_STORE;
    TRY(run_gemm(h, T_GEMM_ENC, T_RED_ENC, g, false, true));
  }
  return 0;
}

// One discriminator update on local rows rows_dev[0..nb) (GANMF.py:131-132,138,186-187).
int d_step(ganmf_handle* h, const int* rows_dev, int nb, int b_global, float* parts, float* arena) {
  float* regWe = arena + 2 * (size_t)h->reg_cap;   // this step's arena slot: seg2 = sum We_ext^2, seg3 = sum Wd_ext^2
  float* regWd = arena + 3 * (size_t)h->reg_cap;
  const int N = h->N, e = h->e;
  const bool dist = h->has_comm;
  // (a staged step has a slot of its own; else the slot alternates: the side lane may still read lr_t of the step before)
  if (dist && !h->front_staged) h->d_alpha = h->d_alpha == S_ALPHA_D ? S_ALPHA_D_ALT : S_ALPHA_D;
  const int aslot = h->d_alpha;
  const float inv_bn = 1.0f / ((float)b_global * (float)N);
  int sqn = 0;
  bool fused = false;
  int regn[2] = {ADAM_GRID, ADAM_GRID};
  if (nb > 0) {
    TRY(step_front(h, rows_dev, nb, 0));
    TRY(dp_join(h, PEND_WD));      // (data-parallel: the previous step's decoder update ran under this step's front and encode GEMM)
    {  // Delta = [E|1].Wd_ext - inp, per-path sum of squares  (GANMF.py:66-68), batch z = path
      GemmP g{};
      g.A = h->E; g.lda = h->lde; g.B = h->Wd.p; g.ldb = h->ldN;
      g.C = h->Dl; g.ldc = h->ldN; g.M = nb; g.N = N; g.K = e + 1;
      g.nbatch = 2; g.a_batch_stride = (long long)nb * h->lde; g.c_batch_stride = (long long)nb * h->ldN;
      g.epi.kind = EPI_SUB_AUX_SQ; g.epi.aux = h->XF; g.epi.ldaux = h->ldN;
      g.epi.aux_batch_stride = (long long)nb * h->ldN; g.epi.sq_partials = h->sqp;
      if (h->sparse_d) {      // the real rows were never expanded: X[m, n] is looked up in the CSR rows of the batch
        g.epi.csr_indptr = h->urm.indptr; g.epi.csr_indices = h->urm.indices; g.epi.csr_data = h->data; g.epi.csr_rows = rows_dev;
      }
      // [real ; generated] are contiguous in E, XF and Dl: with whole 64-row tiles per path the two batches are ONE product of
      // 2.nb rows, whose list order (tile row fastest) puts the four row tiles of a tile column next to each other on one XCD --
      // the decoder panel is fetched once instead of once per batch (rocprofv3 FETCH_SIZE: 42.5 MB per launch as two batches
      // against 23.3 MB algorithmic, profiles/r02_traffic.json).  Same tiles, same K order, partial sums filed per path as before.
      bool merged = false;
      if (!h->sparse_d && nb % 64 == 0) {
        const GemmPlan p1 = gemm_plan(2 * nb, g.N, g.K, 1, true, h->tune), p2 = gemm_plan(g.M, g.N, g.K, 2, true, h->tune);
        if (p1.tile == 64 && p2.tile == 64 && p1.nsplit == 1 && p2.nsplit == 1 && p1.mode == p2.mode && p1.kg == p2.kg && p1.ring == p2.ring) {
          GemmP q = g;
          q.M = 2 * nb; q.nbatch = 1; q.a_batch_stride = 0; q.c_batch_stride = 0; q.epi.aux_batch_stride = 0;
          q.epi.sq_m_half = nb / 64;
          int cnt = 0;
          TRY(run_gemm(h, T_GEMM_DEC, T_RED_DEC, q, false, true, &cnt, 4.0 * 2 * nb * N));
          sqn = p2.sq_count;      // per path, as the two-batch form counts them
          merged = true;
        }
      }
      if (!merged)
      TRY(run_gemm(h, T_GEMM_DEC, T_RED_DEC, g, false, true, &sqn, 4.0 * 2 * nb * N));
    }
  } else {
    // rank out of rows: still open the optimizer step and contribute zeros to the collectives
    GANMF_LAUNCH(open_step_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), 0, aslot, h->cfg.d_lr);
    HIP_TRY(hipGetLastError());
  }
  if (dist) {
    MultiRed mr{};
    mr.count = 2; mr.out = h->scal;
    mr.e[0] = {h->sqp, sqn, S_SUM_REAL, 0};
    mr.e[1] = {h->sqp + sqn, sqn, S_SUM_FAKE, 0};
    {
      Scope s(h, T_MULTIRED, 0, 0);
      GANMF_LAUNCH(multi_reduce_kernel, dim3(S_SUM_FAKE + 1), dim3(256), 0, h->st, mr);      // block = destination slot
      HIP_TRY(hipGetLastError());
    }
    TRY(allreduce(h, h->scal + S_SUM_REAL, 2));
  }
  const DCoefP dc{h->scal, h->sqp, sqn, sqn, dist ? 1 : 0, h->cfg.m, nb, inv_bn, h->E, h->Es, h->lde, h->rs, parts};
  const long long dc_total = (long long)2 * nb * (h->lde / 4);
  // Single GPU, dE split along K: the dE GEMM only writes slabs (its row scale is applied when they are summed, inside the gWd
  // launch), so it does not depend on the hinge scalars and d_coef rides in ITS launch as extra blocks (de_dcoef_kernel).
  bool dcoef_done = false;
  GemmP gde{};
  GemmPlan pde;
  // (data-parallel runs take the same launch: the two sums d_coef needs were all-reduced just above)
  if (nb > 0 && (h->multi & 4) && (h->multi & 8)) {
    gde.A = h->Dl; gde.lda = h->ldN; gde.B = h->Wd.p; gde.ldb = h->ldN;
    gde.C = h->dE; gde.ldc = h->lde; gde.M = 2 * nb; gde.N = e; gde.K = N; gde.nbatch = 1;
    gde.epi.kind = EPI_ROWSCALE; gde.epi.rowscale = h->rs; gde.zero_page = h->zero_page;
    pde = gemm_plan(gde.M, gde.N, gde.K, 1, false, h->tune);
    pde.persist = 0;
    GemmPlan pskn = pde;
    const bool de_stream = h->skinny_n && plan_skinny_n(pskn, gde, false);      // (emb_dim <= 32: dE is a stream over Delta, gemm_skinny.hpp)
    if (!de_stream && plan_is_f32_64_kg(pde, 4) && pde.nsplit > 1) {
      TRY(ensure_slab(h, gemm_slab_elems(pde, gde.M, gde.ldc, 1), 0));
      Scope s(h, T_DE_DCOEF, gemm_flops(gde.M, gde.N, gde.K), gemm_bytes(gde.M, gde.N, gde.K) + 8.0 * 2 * nb * e);
      GemmP q = gde;
      fill_plan(q, pde);
      q.C = h->slab; q.c_split_stride = (long long)gde.M * gde.ldc; q.c_batch_stride = (long long)gde.M * gde.ldc;
      const int ng = pde.tiles_m * pde.tiles_n * pde.nsplit;
      const int nd = 0;      // (d_coef is shared out over the GEMM's workgroups, no extra ones)
      if (combined_x3(h)) GANMF_LAUNCH((de_dcoef_kernel<4, true>), dim3(ng + nd), dim3(1024), 0, h->st, q, dc, nd);
      else GANMF_LAUNCH(de_dcoef_kernel<4>, dim3(ng + nd), dim3(1024), 0, h->st, q, dc, nd);
      HIP_TRY(hipGetLastError());
      dcoef_done = true;
    }
  }
  if (!dcoef_done) {
    Scope s(h, T_DCOEF, 0, 8.0 * 2 * nb * e);
    const int grid = (int)std::max<long long>(1, std::min<long long>(128, (dc_total + 1023) / 1024));
    GANMF_LAUNCH(d_coef_kernel, dim3(grid), dim3(256), 0, h->st, dc);
    HIP_TRY(hipGetLastError());
  }
  if (nb > 0) {
    const bool regD = h->cfg.d_reg != 0.f;
    fused = !dist;      // single GPU: Adam runs in the epilogue of the weight-gradient GEMMs
    GemmTune ft;
    ft.tile = FUSED_TILE; ft.ring = 2; ft.nsplit = 1;
    ft.mode = h->tune.mode != MFMA_AUTO ? h->tune.mode : FUSED_MODE;
    ft.bk = FUSED_BK;
    // the data-parallel path runs the same two GEMMs with a plain store epilogue: same tile, split and arithmetic,
    // so that it stays bitwise equal to the fused single-GPU path (tests/test_gpu_parity.py, one-rank RCCL)
    const GemmTune* wg_tune = &ft;
    // sparse regime: the encoder-gradient GEMM runs over the generated rows only (A = F, B = dE_f, K = nb); the real rows' share
    // X^T . dE_r (and the bias row's column sums of dE_r) is added in its epilogue from the CSC matrix, before Adam / the store
    const int start = (int)(rows_dev - h->perm);      // position of this batch in the epoch permutation (pos[] is its inverse)
    auto sparse_gWe = [&](GemmP& g) {
      if (!h->sparse_d) return;
      g.A = h->XF + (size_t)nb * h->ldN; g.B = h->dE + (size_t)nb * h->lde; g.K = nb;
      g.epi.sp_rows = h->sp_rows; g.epi.sp_ld = h->lde; g.epi.sp_bias_row = N; g.epi.sp_bias_parts = CSC_BIAS_PARTS;
    };
    auto sparse_rows = [&]() -> int {      // S = X^T . dE_r (+ the bias parts): dE must be final
      if (!h->sparse_d) return 0;
      Scope s(h, T_DENSIFY, 0, 4.0 * ((double)h->urm.nnz / std::max(h->U, 1) * nb * e + 2.0 * (N + CSC_BIAS_PARTS) * e));
      GANMF_LAUNCH(csc_rows_kernel, dim3(N + CSC_BIAS_PARTS), dim3(256), 0, h->st, h->csc.indptr.get(), h->csc.indices.get(), h->csc_val.get(),
                   h->pos, start, nb, N, h->dE.get(), h->lde, e, h->sp_rows.get());
      HIP_TRY(hipGetLastError());
      return 0;
    };
    RedP dE_red{};                  // single GPU: the slab sum of dE rides in the gWd launch (gWd does not read dE, gWe does)
    auto gemm_gWd = [&]() -> int {  // gWd_ext = (rs*[E|1])^T . Delta   -> rows 0..e-1 = gWd, row e = gbd
      GemmP g{};
      g.A = h->Es; g.lda = h->lde; g.B = h->Dl; g.ldb = h->ldN;
      g.C = h->Wd.g; g.ldc = h->ldN; g.M = e + 1; g.N = N; g.K = 2 * nb; g.epi.kind = EPI_STORE;
      g.a_scale = grad_scale(h, b_global);     // Es = rs (.) E carries the 2/(B.N) of the loss gradient
      if (fused) {
        g.epi.kind = EPI_ADAM; g.epi.adam_theta = h->Wd.p; g.epi.adam_m = h->Wd.m; g.epi.adam_v = h->Wd.v;
        g.epi.adam_alpha = h->scal + aslot; g.epi.adam_reg = h->cfg.d_reg;
        g.epi.sq_partials = regD ? regWd : nullptr;
      }
      return run_gemm(h, T_GEMM_GWD, T_RED_GWD, g, true, true, &regn[1], fused ? 24.0 * h->Wd.count() : 0, 0, wg_tune, nullptr,
                      nullptr, dE_red.part ? &dE_red : nullptr);
    };
    // Data-parallel: ONE order of collectives whatever this rank's row count or GEMM plans (ranks of a ragged step plan
    // differently; a rank without rows issues the same sequence on zero gradients): encoder first -- the next step needs We one
    // GEMM earlier than Wd.  dE (its slabs may exist already, de_dcoef_kernel) -> gWe_ext -> We's reduce-scatter / Adam slice /
    // all-gather on the side lane under the gWd_ext GEMM and the next step's row expansion + generator GEMM (joined before its
    // encode GEMM) -> gWd_ext -> Wd's behind them under that encode GEMM (joined before the decode GEMM; dE has read the old
    // decoder long before).
    if (dcoef_done) {   // the slabs are there already: hand their sum (+ row scale) to the gWd launch
      dE_red = RedP{};
      dE_red.part = h->slab; dE_red.nsplit = pde.nsplit; dE_red.out = gde.C; dE_red.ld = gde.ldc; dE_red.M = gde.M; dE_red.N = gde.N;
      dE_red.batch_stride = 0; dE_red.epi = gde.epi; dE_red.epi.sq_stride = GEMM_RED_GRID;      // (no partials: EPI_ROWSCALE)
      dE_red.split_stride = (long long)gde.M * gde.ldc;
    } else {  // dE = rs * (Delta . Wd^T)          (bias row e of Wd_ext is not part of this product; reads the OLD Wd)
      GemmP g{};
      g.A = h->Dl; g.lda = h->ldN; g.B = h->Wd.p; g.ldb = h->ldN;
      g.C = h->dE; g.ldc = h->lde; g.M = 2 * nb; g.N = e; g.K = N;
      g.epi.kind = EPI_ROWSCALE; g.epi.rowscale = h->rs;
      TRY(run_gemm(h, T_GEMM_DE, T_RED_DE, g, false, false, nullptr, 0, 0, nullptr, nullptr,
                   (!dist && (h->multi & 4)) ? &dE_red : nullptr));
    }
    // Weight-gradient GEMMs.  Single GPU: the gradient tile never leaves the CU -- the epilogue
    // applies TF-Adam to theta/m/v in place (after dE, which reads the old decoder).
    // Data-parallel: the gradients are stored, reduce-scattered, and each rank updates its slice (dp_update).
    bool wpair = false;
    if (fused && (h->multi & 16) && dE_red.part) {
      // both weight-gradient products in ONE launch (wgrad_pair_kernel); the slab sum of dE, which gWe reads, gets its own
      // launch in front
      GemmP g0{}, g1{};
      g0.A = h->Es; g0.lda = h->lde; g0.B = h->Dl; g0.ldb = h->ldN;
      g0.C = h->Wd.g; g0.ldc = h->ldN; g0.M = e + 1; g0.N = N; g0.K = 2 * nb; g0.nbatch = 1; g0.zero_page = h->zero_page;
      g0.a_scale = grad_scale(h, b_global);
      g0.epi.kind = EPI_ADAM; g0.epi.adam_theta = h->Wd.p; g0.epi.adam_m = h->Wd.m; g0.epi.adam_v = h->Wd.v;
      g0.epi.adam_alpha = h->scal + aslot; g0.epi.adam_reg = h->cfg.d_reg; g0.epi.sq_partials = regD ? regWd : nullptr;
      g1.A = h->XF; g1.lda = h->ldN; g1.B = h->dE; g1.ldb = h->lde;
      g1.C = h->We.g; g1.ldc = h->lde; g1.M = N + 1; g1.N = e; g1.K = 2 * nb; g1.nbatch = 1; g1.zero_page = h->zero_page;
      g1.b_scale = grad_scale(h, b_global);
      g1.epi.kind = EPI_ADAM; g1.epi.adam_theta = h->We.p; g1.epi.adam_m = h->We.m; g1.epi.adam_v = h->We.v;
      g1.epi.adam_alpha = h->scal + aslot; g1.epi.adam_reg = h->cfg.d_reg; g1.epi.sq_partials = regD ? regWe : nullptr;
      sparse_gWe(g1);
      GemmPlan p0 = gemm_plan(g0.M, g0.N, g0.K, 1, regD, ft, true), p1 = gemm_plan(g1.M, g1.N, g1.K, 1, regD, ft, true);
      auto staged = [](const GemmPlan& pl) { return pl.mode == MFMA_BF16X3 && pl.tile == 64 && pl.bk == 32 && pl.nsplit == 1; };
      if (staged(p0) && staged(p1)) {
        {
          Scope s(h, T_RED_DE, 0, 4.0 * (dE_red.nsplit + 1) * dE_red.M * dE_red.N);
          GANMF_LAUNCH(splitk_reduce_kernel, dim3(GEMM_RED_GRID, 1), dim3(256), 0, h->st, dE_red);
          HIP_TRY(hipGetLastError());
        }
        TRY(sparse_rows());
        fill_plan(g0, p0);
        fill_plan(g1, p1);
        g0.n_fastest = g1.n_fastest = 1;
        // gWd's tiles in XCD-blocked order (tile_coords): an XCD takes a band of tile COLUMNS -- its eighth of Delta instead of all of it
        // through its L2 -- and walks it tile row fastest; gWe's column-fastest list already gives every XCD a band of X rows
        if (h->wgrad_xb > 0) { g0.n_fastest = 0; g0.xb_m = 1; g0.xb_n = 8; g0.xb_band = h->wgrad_xb; }
        regn[1] = p0.sq_count; regn[0] = p1.sq_count;
        const int n0 = p0.tiles_m * p0.tiles_n, n1 = p1.tiles_m * p1.tiles_n;
        {
          Scope s(h, T_WPAIR, gemm_flops(g0.M, g0.N, g0.K) + gemm_flops(g1.M, g1.N, g1.K),
                  // operands once + the six Adam streams; the gradients themselves never reach HBM
                  4.0 * ((double)g0.K * (g0.M + g0.N) + (double)g1.K * (g1.M + g1.N)) + 24.0 * ((double)g0.M * g0.N + (double)g1.M * g1.N));
          GANMF_LAUNCH(wgrad_pair_kernel, dim3(n0 + n1), dim3(256), 0, h->st, g0, g1);
          HIP_TRY(hipGetLastError());
        }
        wpair = true;
      }
    }
    if (dist && dE_red.part) {     // (dcoef_done: the slabs of dE are waiting for their sum)
      Scope s(h, T_RED_DE, 0, 4.0 * (dE_red.nsplit + 1) * dE_red.M * dE_red.N);
      GANMF_LAUNCH(splitk_reduce_kernel, dim3(GEMM_RED_GRID, 1), dim3(256), 0, h->st, dE_red);
      HIP_TRY(hipGetLastError());
      dE_red.part = nullptr;      // (summed: nothing to attach to the gWd launch)
    }
    if (!dist && !wpair) TRY(gemm_gWd());
    if (!wpair) {  // gWe_ext = [X;F | 1]^T . dE       -> rows 0..N-1 = gWe, row N = gbe
      TRY(sparse_rows());
      GemmP g{};
      g.A = h->XF; g.lda = h->ldN; g.B = h->dE; g.ldb = h->lde;
      g.C = h->We.g; g.ldc = h->lde; g.M = N + 1; g.N = e; g.K = 2 * nb; g.epi.kind = EPI_STORE;
      g.b_scale = grad_scale(h, b_global);     // dE
      if (fused) {
        g.epi.kind = EPI_ADAM; g.epi.adam_theta = h->We.p; g.epi.adam_m = h->We.m; g.epi.adam_v = h->We.v;
        g.epi.adam_alpha = h->scal + aslot; g.epi.adam_reg = h->cfg.d_reg;
        g.epi.sq_partials = regD ? regWe : nullptr;
      }
      sparse_gWe(g);
      const bool armed = dist && fork_arm(h);
      TRY(run_gemm(h, T_GEMM_GWE, T_RED_GWE, g, true, true, &regn[0], fused ? 24.0 * h->We.count() : 0, 0, wg_tune));
      if (dist) TRY(fork_wait(h, armed));       // the side lane waits for gWe_ext
    }
    if (dist) {
      TRY(dp_update(h, T_ADAM_D, h->We, aslot, h->cfg.d_reg, regD ? regWe : nullptr, 1));
      TRY(dp_mark(h, PEND_WE));
      const bool armed = fork_arm(h);
      TRY(gemm_gWd());
      TRY(fork_wait(h, armed));       // ... and for gWd_ext
      TRY(dp_update(h, T_ADAM_D, h->Wd, aslot, h->cfg.d_reg, regD ? regWd : nullptr, 1));
      TRY(dp_mark(h, PEND_WD));
      (void)regn; (void)parts;
      return 0;
    }
  } else {
    // (ranks with rows join inside step_front; the previous step's encoder update may still be reducing We.g on the side lane)
    TRY(dp_join(h));
    HIP_TRY(hipMemsetAsync(h->gD, 0, h->gD_elems * sizeof(float), h->st));
    if (dist) {   // same collective order as the ranks that have rows: encoder, then decoder
      const bool regD = h->cfg.d_reg != 0.f;
      TRY(lane_fork(h));
      TRY(dp_update(h, T_ADAM_D, h->We, aslot, h->cfg.d_reg, regD ? regWe : nullptr, 1));
      TRY(dp_mark(h, PEND_WE));
      TRY(dp_update(h, T_ADAM_D, h->Wd, aslot, h->cfg.d_reg, regD ? regWd : nullptr, 1));
      TRY(dp_mark(h, PEND_WD));
    }
  }
  const bool reg = h->cfg.d_reg != 0.f;
  if (!dist && !fused) {
    TRY(adam_dense(h, T_ADAM_D, h->We, h->We.g, aslot, h->cfg.d_reg, reg ? regWe : nullptr));
    TRY(adam_dense(h, T_ADAM_D, h->Wd, h->Wd.g, aslot, h->cfg.d_reg, reg ? regWd : nullptr));
  }
  (void)regn; (void)parts;
  return 0;   // the sum(theta^2) partials are reduced once per epoch (finish_parts_kernel)
}

// ---- generator pass with ONE all-rows update of user_embeddings (kernels.hpp: adam_rows_advance_kernel / adam_rows_flush_kernel) -----------
inline int lazy_tab_slot(const ganmf_handle* h, int p) { return S_TAB + (2 + (p & 1)) * h->tab_cap; }
bool lazy_pass_ok(const ganmf_handle* h, int64_t per_pass, int64_t n) {
  if (!(h->lazy_rows && h->cfg.g_reg == 0.f && per_pass >= 4 && per_pass <= h->tab_cap && n > 0)) return false;
  // the pass keeps every step's gUb slabs until its flush: never more than a quarter of the free device memory beyond what the arena holds
  const GemmPlan pl = gemm_plan(h->B, h->k, h->N, 1, false, h->tune);
  const size_t per_step = (size_t)(std::max(pl.nsplit, 1) + 1) * h->B * h->ldk + 128;
  size_t have = 0;
  for (const auto& ch : h->lazy_chunks) have += ch.cap;
  const size_t need = (size_t)per_pass * per_step;
  if (need <= have) return true;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  return (need - have) * sizeof(float) <= free_b / 4;
}
// a block of the pass arena (64-float aligned); chunks are kept for the passes to come
int lazy_block(ganmf_handle* h, size_t elems, float** out) {
  elems = (elems + 63) / 64 * 64;
  while (h->lazy_chunk < h->lazy_chunks.size() && h->lazy_used + elems > h->lazy_chunks[h->lazy_chunk].cap) { ++h->lazy_chunk; h->lazy_used = 0; }
  if (h->lazy_chunk == h->lazy_chunks.size()) {
    const size_t want = std::max<size_t>(elems, (size_t)16 << 20);      // 64 MiB chunks, zeroed (lazy_chunk_alloc)
    if (!lazy_chunk_alloc(h, want)) HIP_TRY(hipErrorOutOfMemory);
    h->lazy_used = 0;
  }
  *out = h->lazy_chunks[h->lazy_chunk] + h->lazy_used;
  h->lazy_used += elems;
  return 0;
}
void lazy_pass_abort(ganmf_handle* h) {
  h->lazy_pass = false; h->Ub = h->Ub_own; h->gUb = h->gUb_own; h->g_alpha = S_ALPHA_G;
}
int lazy_pass_begin(ganmf_handle* h, int p, int64_t per_pass, int64_t n, bool opened) {      // opened: lr_t of the pass's steps is in its table already (stage_pass)
  const size_t need = (size_t)n * h->ldk;
  if (need > h->Ub_sched.cap) {
    HIP_TRY(hipStreamSynchronize(h->st2));
    TRY(h->Ub_sched.grow(h->st, need, true));
  }
  const int tab = lazy_tab_slot(h, p);
  if (!opened) {
    GANMF_LAUNCH(open_steps_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), 1, tab, (int)per_pass, h->cfg.g_lr);
    HIP_TRY(hipGetLastError());
  }
  {
    Scope s(h, T_ADAM_U, 0, 16.0 * n * h->ldk);
    const long long total = (long long)n * (h->ldk / 4);
    const int grid = (int)std::max<long long>(1, std::min<long long>(8192, (total + 255) / 256));
    GANMF_LAUNCH(adam_rows_advance_kernel, dim3(grid), dim3(256), 0, h->st, h->Ue.p.get(), h->Ue.m.get(), h->Ue.v.get(), h->perm.get(), h->pos_step, (int)n,
                 h->ldk, h->scal.get(), tab, h->cfg.g_reg, h->Ub_sched.get());
    HIP_TRY(hipGetLastError());
  }
  h->lazy_steps.assign((size_t)per_pass, LazyStep{nullptr, 0, 1, 0, 0});
  h->lazy_chunk = 0; h->lazy_used = 0;
  h->lazy_pass = true;
  return 0;
}
int lazy_pass_end(ganmf_handle* h, int p, int64_t per_pass) {
  const size_t T = (size_t)per_pass;
  if (2 * T > h->lazy_stage.cap) TRY(h->lazy_stage.grow(h->st, 2 * (T + 16), false));
  if (2 * T > h->lazy_tab.cap) TRY(h->lazy_tab.grow(h->st, 2 * (T + 16), false));
  if (p >= 2) HIP_TRY(hipStreamSynchronize(h->st));      // the half of the staging table this pass reuses has been copied
  LazyStep* const host = h->lazy_stage + (size_t)(p & 1) * (h->lazy_stage.cap / 2);
  LazyStep* const dev = h->lazy_tab + (size_t)(p & 1) * (h->lazy_tab.cap / 2);
  std::copy(h->lazy_steps.begin(), h->lazy_steps.end(), host);
  HIP_TRY(hipMemcpyAsync(dev, host, T * sizeof(LazyStep), hipMemcpyHostToDevice, h->st));
  {
    Scope s(h, T_ADAM_U, 0, 24.0 * h->Ue.count());
    // one float4 per thread in ONE round (the T-step loop per element is all arithmetic: a second grid-stride round with half the threads
    // busy would double the launch)
    const long long total = (long long)h->U * (h->ldk / 4);
    const int grid = (int)std::max<long long>(1, std::min<long long>(8192, (total + 255) / 256));
    GANMF_LAUNCH(adam_rows_flush_kernel, dim3(grid), dim3(256), 0, h->st, h->Ue.p.get(), h->Ue.m.get(), h->Ue.v.get(), h->pos, h->pos_step, dev,
                 (int)per_pass, h->U, h->ldk, h->scal.get(), lazy_tab_slot(h, p), h->cfg.g_reg);
    HIP_TRY(hipGetLastError());
  }
  lazy_pass_abort(h);      // (restores the handle's own minibatch buffers and lr_t slot)
  return 0;
}

// Generator parameter update shared by GANMF and DisGANMF: gUb = dF.V (reads the OLD V), gV = dF^T.Ub,
// Adam on V (fused into the gV GEMM epilogue on a single GPU) and the all-rows Adam on U.
// *regn_v = number of sum(V^2) partials written (when g_reg != 0).
int gen_update(ganmf_handle* h, int nb, int start, int b_global, int* regn_v, float* reg_u, float* reg_v) {
  const int N = h->N, k = h->k;
  const bool reg = h->cfg.g_reg != 0.f;
  const bool dist = h->has_comm;
  const bool fused = !dist && nb > 0;
  *regn_v = ADAM_GRID;
  const bool lazy = h->lazy_pass;      // the step's gUb (or its slabs) stays in the pass arena until the pass's flush (lazy_pass_end)
  h->gub_x3 = (long long)((N + 63) / 64) * ((k + 63) / 64) >= 2 * GEMM_CUS;      // (= staged_gv below)
  SlabRef gub{h->gUb, 1, 0};
  auto gemm_gUb = [&]() -> int {  // gUb = dF . V     (reads the OLD V)
    GemmP g{};
    g.A = h->dF; g.lda = h->ldN; g.B = h->V.p; g.ldb = h->ldk;
    g.C = h->gUb; g.ldc = h->ldk; g.M = nb; g.N = k; g.K = N; g.epi.kind = EPI_STORE;
    g.a_scale = grad_scale(h, b_global);      // dF
    if (!lazy) return run_gemm(h, T_GEMM_GUB, T_RED_GUB, g, false, true, nullptr, 0, 0, nullptr, h->defer_gub ? &gub : nullptr);   // slabs summed by adam_rows_kernel
    // lazy pass: the final matrix and (when the consumer sums them) the slabs go to blocks of the pass arena
    const GemmPlan pl = plan_gemm(h, T_GEMM_GUB, g, false, true, nullptr);
    float* fin = nullptr;
    TRY(lazy_block(h, (size_t)nb * h->ldk, &fin));
    g.C = fin;
    gub = SlabRef{fin, 1, 0};
    if (pl.nsplit > 1 && h->defer_gub) {
      const size_t elems = gemm_slab_elems(pl, g.M, g.ldc, 1);
      float* blk = nullptr;
      TRY(lazy_block(h, elems, &blk));
      h->slab2_lent = blk; h->slab2_lent_elems = elems;      // (run_gemm files deferred slabs in the second workspace)
    }
    const int rc = run_gemm(h, T_GEMM_GUB, T_RED_GUB, g, false, true, nullptr, 0, 0, nullptr, h->defer_gub ? &gub : nullptr, nullptr, nullptr, &pl);
    h->slab2_lent = nullptr; h->slab2_lent_elems = 0;
    return rc;
  };
  auto gemm_gV = [&]() -> int {   // gV = dF^T . Ub
    GemmP g{};
    g.A = h->dF; g.lda = h->ldN; g.B = h->Ub; g.ldb = h->ldk;
    g.C = h->V.g; g.ldc = h->ldk; g.M = N; g.N = k; g.K = nb; g.epi.kind = EPI_STORE;
    g.a_scale = grad_scale(h, b_global);      // dF
    if (fused) {
      g.epi.kind = EPI_ADAM; g.epi.adam_theta = h->V.p; g.epi.adam_m = h->V.m; g.epi.adam_v = h->V.v;
      g.epi.adam_alpha = h->scal + h->g_alpha; g.epi.adam_reg = h->cfg.g_reg;
      g.epi.sq_partials = reg ? reg_v : nullptr;
      g.adam_touch = adam_touch_for(h, g.M, g.ldc);
    }
    GemmTune ft;
    ft.tile = 64; ft.ring = 2; ft.nsplit = 1;
    ft.mode = h->tune.mode != MFMA_AUTO ? h->tune.mode : FUSED_MODE;
    ft.bk = FUSED_BK;
    // the half-depth staged split-bf16 kernel of the other fused-Adam GEMMs once the output has at least two 64 x 64 tiles per
    // CU (C4 width, N = 50 000: 136 -> 102 us, +2 .. 5 % steps/s); below that the fp32 ring kernel (C2: 17.2 vs 18.1 us, and it
    // pairs with gUb in one launch).
    const long long gv_tiles = (long long)((N + 63) / 64) * ((k + 63) / 64);
    const bool staged_gv = gv_tiles >= 2 * GEMM_CUS;
    TRY(run_gemm(h, T_GEMM_GV, T_RED_GV, g, true, true, regn_v, fused ? 24.0 * h->V.count() : 0, 0, staged_gv ? &ft : nullptr));
    if (!fused) *regn_v = ADAM_GRID;
    return 0;
  };
  // gUb and gV in ONE launch (pair_kernel): both read dF.  Single GPU: gUb reads the old V while gV's Adam epilogue writes the
  // new V into the second buffer, swapped in afterwards.  Data-parallel: gV is stored (it must be reduced before its Adam), V is
  // not touched inside the launch.  Only when both are planned onto the 16-wave fp32 ring kernel.
  bool paired = false, pair_armed = false;
  // Data-parallel, generator pass with the per-pass update of U (lazy): nothing is left on the main lane between this launch and the next
  // step's generator GEMM, which reads the new V -- V's reduce-scatter / Adam slice / all-gather then run ON the main lane: a fork and a
  // join around a chain that nothing overlaps cost it 5-8 us each (profiles/r04_dp_timeline.md: 31 us from the end of this launch to the
  // next generator launch for 16 us of kernels).
  const bool v_inline = dist && lazy;
  if (nb > 0 && (fused || dist) && (h->multi & 2) && h->defer_gub && h->V_alt) {
    if (dist) TRY(dp_join(h));
    GemmP g0{}, g1{};
    g0.A = h->dF; g0.lda = h->ldN; g0.B = h->V.p; g0.ldb = h->ldk;
    g0.C = h->gUb; g0.ldc = h->ldk; g0.M = nb; g0.N = k; g0.K = N; g0.epi.kind = EPI_STORE; g0.nbatch = 1;
    g0.zero_page = h->zero_page; g0.a_scale = grad_scale(h, b_global);
    g1.A = h->dF; g1.lda = h->ldN; g1.B = h->Ub; g1.ldb = h->ldk;
    g1.C = h->V.g; g1.ldc = h->ldk; g1.M = N; g1.N = k; g1.K = nb; g1.nbatch = 1;
    g1.zero_page = h->zero_page; g1.a_scale = grad_scale(h, b_global);
    g1.epi.kind = EPI_STORE;
    if (fused) {
      g1.epi.kind = EPI_ADAM; g1.epi.adam_theta = h->V.p; g1.epi.adam_theta_out = h->V_alt; g1.epi.adam_m = h->V.m; g1.epi.adam_v = h->V.v;
      g1.epi.adam_alpha = h->scal + h->g_alpha; g1.epi.adam_reg = h->cfg.g_reg;
      g1.epi.sq_partials = reg ? reg_v : nullptr;
    }
    GemmPlan p0 = gemm_plan(g0.M, g0.N, g0.K, 1, false, h->tune);
    GemmPlan p1 = gemm_plan(g1.M, g1.N, g1.K, 1, g1.epi.sq_partials != nullptr, h->tune, true);
    // (a low-precision handle: both products on the 16-wave one-piece loop they would run stand-alone -- pair_lp_kernel)
    const bool pair_lp = (h->x3kg & 4) && low_precision(h) && plan_is_lp_64(p0) && plan_is_lp_64(p1) && p0.mode == p1.mode;
    if (((plan_is_f32_64_kg(p0, 4) && plan_is_f32_64_kg(p1, 4)) || pair_lp) && p1.nsplit == 1 &&
        reduce_groups((long long)g0.M * ((g0.N + 3) >> 2), p0.nsplit) == 1) {
      if (p0.nsplit > 1) {
        const size_t elems = gemm_slab_elems(p0, g0.M, g0.ldc, 1);
        float* dst = nullptr;
        if (lazy) TRY(lazy_block(h, elems, &dst));
        else { TRY(ensure_slab(h, elems, 1)); dst = h->slab2; }
        g0.C = dst; g0.c_split_stride = (long long)g0.M * g0.ldc;
        gub = SlabRef{dst, p0.nsplit, (long long)g0.M * g0.ldc};
      } else if (lazy) {
        float* dst = nullptr;
        TRY(lazy_block(h, (size_t)g0.M * g0.ldc, &dst));
        g0.C = dst;
        gub = SlabRef{dst, 1, 0};
      }
      g0.c_batch_stride = (long long)g0.M * g0.ldc;
      fill_plan(g0, p0);
      fill_plan(g1, p1);
      if (fused) g1.n_fastest = 1;
      if (fused) g1.adam_touch = adam_touch_for(h, g1.M, g1.ldc);
      if (fused) *regn_v = p1.sq_count;
      const int n0 = p0.tiles_m * p0.tiles_n * p0.nsplit, n1 = p1.tiles_m * p1.tiles_n;
      {
        Scope s(h, T_PAIR, gemm_flops(g0.M, g0.N, g0.K) + gemm_flops(g1.M, g1.N, g1.K),
                gemm_bytes(g0.M, g0.N, g0.K) + gemm_bytes(g1.M, g1.N, g1.K) + (fused ? 24.0 * h->V.count() : 0));
        pair_armed = dist && !v_inline && fork_arm(h);
        if (pair_lp && p0.mode == MFMA_F16) GANMF_LAUNCH(pair_lp_kernel<true>, dim3(n0 + n1), dim3(1024), 0, h->st, g0, g1);
        else if (pair_lp) GANMF_LAUNCH(pair_lp_kernel<false>, dim3(n0 + n1), dim3(1024), 0, h->st, g0, g1);
        else GANMF_LAUNCH((pair_kernel<4, 2>), dim3(n0 + n1), dim3(1024), 0, h->st, g0, g1);
        HIP_TRY(hipGetLastError());
      }
      if (fused) std::swap(h->V.p, h->V_alt);
      paired = true;
    }
  }
  if (dist && paired && v_inline) {
    TRY(dp_update(h, T_ADAM_V, h->V, h->g_alpha, h->cfg.g_reg, reg ? reg_v : nullptr, 0));
  } else if (dist && paired) {
    // the whole update of V on the side lane, under the all-rows Adam pass over U (which reads neither V nor its gradient)
    TRY(fork_wait(h, pair_armed));
    TRY(dp_update(h, T_ADAM_V, h->V, h->g_alpha, h->cfg.g_reg, reg ? reg_v : nullptr, 1));
  } else if (dist) {
    // data-parallel, separate launches: gV first; its reduce-scatter runs on the side lane under gUb (which reads the OLD V),
    // the Adam slice and the all-gather of V under the all-rows Adam pass over U
    TRY(dp_join(h));
    if (nb > 0) TRY(gemm_gV());
    else HIP_TRY(hipMemsetAsync(h->V.g, 0, h->V.cap * sizeof(float), h->st));
    TRY(lane_fork(h));
    TRY(reduce_scatter(h, h->V.g, h->V.cap, 1, T_COLL_V));
    if (nb > 0) TRY(gemm_gUb());
    TRY(lane_fork(h));
    const size_t slice = h->V.cap / (size_t)h->cfg.world_size, off = (size_t)h->cfg.rank * slice;
    TRY(adam_dense(h, T_ADAM_V, h->V, h->V.g, h->g_alpha, h->cfg.g_reg, reg ? reg_v : nullptr, 1, off, slice));
    TRY(all_gather(h, h->V.p, h->V.cap, 1, T_COLL_V));
  } else if (nb > 0) {
    if (!paired) {
      TRY(gemm_gUb());
      TRY(gemm_gV());      // fused: Adam(V) in the epilogue, after gUb has read the old V
    }
  } else {
    HIP_TRY(hipMemsetAsync(h->V.g, 0, h->V.padded() * sizeof(float), h->st));
  }
  if (lazy) {      // the pass's flush sums this step's slabs and applies the update (adam_rows_flush_kernel)
    h->lazy_steps[h->lazy_step] = LazyStep{gub.p, gub.split_stride, gub.nsplit, start, nb};
  } else {
    Scope s(h, T_ADAM_U, 0, 24.0 * h->Ue.count());
    GANMF_LAUNCH(adam_rows_kernel, dim3(ADAM_GRID), dim3(256), 0, h->st, h->Ue.p.get(), h->Ue.m.get(), h->Ue.v.get(), gub.p,
                       gub.nsplit, gub.split_stride, h->pos, start, nb, h->U, h->ldk, h->scal.get(), h->g_alpha, h->cfg.g_reg,
                       reg ? reg_u : nullptr);
    HIP_TRY(hipGetLastError());
  }
  if (dist) {      // V is read by the very next kernel of the next step (generator GEMM)
    if (!(paired && v_inline)) { Scope s(h, T_JOIN_V, 0, 0); TRY(lane_join(h)); }
  } else if (!fused) TRY(adam_dense(h, T_ADAM_V, h->V, h->V.g, h->g_alpha, h->cfg.g_reg, reg ? reg_v : nullptr));
  return 0;
}

// One generator update (GANMF.py:133-135,139,200-201).  `start` = position of the batch in the
// epoch permutation (adam_rows_kernel finds batch rows through pos[]).
int g_step(ganmf_handle* h, const int* rows_dev, int nb, int start, int b_global, float* parts, float* arena) {
  // this step's arena slot: seg0 = sum Delta_f^2, seg1 = sum (Ef-Er)^2, seg2 = sum U^2, seg3 = sum V^2 partials
  const size_t cap = h->reg_cap;
  const int N = h->N, e = h->e;
  const float alpha = h->cfg.recon_coefficient;
  const float inv_bn = 1.0f / ((float)b_global * (float)N);
  int sqn = 0, fmn = 0;
  if (nb > 0) {
    TRY(step_front(h, rows_dev, nb, 1));
    TRY(dp_join(h, PEND_WD));
    {  // Delta_f = [Ef|1].Wd_ext - F, sum of squares
      GemmP g{};
      g.A = h->E + (size_t)nb * h->lde; g.lda = h->lde; g.B = h->Wd.p; g.ldb = h->ldN;
      g.C = h->Dl; g.ldc = h->ldN; g.M = nb; g.N = N; g.K = e + 1;
      g.epi.kind = EPI_SUB_AUX_SQ; g.epi.aux = h->XF + (size_t)nb * h->ldN; g.epi.ldaux = h->ldN;
      g.epi.sq_partials = arena;
      TRY(run_gemm(h, T_GEMM_DEC, T_RED_DEC, g, false, true, &sqn, 4.0 * nb * N));
    }
    // host constants: rsG = (1-alpha)*2/(B*N) ; cfm = alpha*2/(B*e)
    const float rsv = (1.0f - alpha) * (2.0f * inv_bn);
    const float cfm = alpha * 2.0f / ((float)b_global * (float)e);
    {  // dE = rsG*(Delta_f . Wd^T) + cfm*(Ef - Er) ; FM partials
      GemmP g{};
      g.A = h->Dl; g.lda = h->ldN; g.B = h->Wd.p; g.ldb = h->ldN;
      g.C = h->dE; g.ldc = h->lde; g.M = nb; g.N = e; g.K = N;
      g.epi.kind = EPI_G_DE; g.epi.c = rsv; g.epi.cfm = cfm;
      g.epi.er = h->E; g.epi.ef = h->E + (size_t)nb * h->lde; g.epi.sq_partials = arena + cap;
      TRY(run_gemm(h, T_GEMM_DE, T_RED_DE, g, false, false, &fmn));
    }
    {  // dF = dE . We^T - rsG*Delta_f      (MSE gradient reaches F through both arguments)
      GemmP g{};
      g.A = h->dE; g.lda = h->lde; g.B = h->We.p; g.ldb = h->lde;
      g.C = h->dF; g.ldc = h->ldN; g.M = nb; g.N = N; g.K = e;
      g.epi.kind = EPI_SUB_SCALED_AUX; g.epi.c = rsv; g.epi.aux = h->Dl; g.epi.ldaux = h->ldN;
      g.a_scale = grad_scale(h, b_global);     // dE
      TRY(run_gemm(h, T_GEMM_DF, T_RED_DF, g, false, false, nullptr, 4.0 * nb * N));
    }
  } else if (!h->lazy_pass) {      // (a lazy pass opened all its steps at once)
    GANMF_LAUNCH(open_step_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), 1, h->g_alpha, h->cfg.g_lr);
    HIP_TRY(hipGetLastError());
  }
  const bool reg = h->cfg.g_reg != 0.f;
  int regn_v = ADAM_GRID;
  TRY(gen_update(h, nb, start, b_global, &regn_v, arena + 2 * cap, arena + 3 * cap));
  (void)parts; (void)reg; (void)sqn; (void)fmn;
  return 0;
}

