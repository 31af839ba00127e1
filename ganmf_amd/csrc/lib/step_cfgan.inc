// step_cfgan.inc -- CFGAN: generator and discriminator MLPs, the masked D-step and G-step, scoring (CFGAN.py:49-176,342-368)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// =================================================================================================
// Discriminator: the handle's DisGANMF members.  Its input block DX [2B, ldx] holds [c | x | 1]: Wl[0] is [2N + 1, e] (condition rows,
// input rows, bias row), so layer 0 is ONE K = 2N + 1 product and both bias and the concat of CFGAN.py:57 ride in it.  Generator:
// CfganState::gen (profile_mlp.inc).  Every dense product goes through run_gemm under the handle's planner; every parameter gradient is a TN product that ends
// in the fused TF-Adam epilogue (EPI_ADAM) -- the output unit's rides in dis_dz_top_kernel as in DisGANMF -- so no gradient is stored.
// Products that read a parameter run before the product that updates it.  sum(theta^2) of the loss is taken at the head of the step
// (sumsq_tensors), at the pre-update parameters like every other term of the reported loss.
// =================================================================================================
int cfgan_create(ganmf_handle* h) {
  const int N = h->N, e = h->e, B = h->B;
  if (low_precision(h)) return fail(-1, "ganmf_create: GANMF_MODEL_CFGAN runs the fp32-accurate products only (GANMF_MFMA asks for bf16 / f16)");
  h->L = h->cfg.d_layers; h->act = h->cfg.d_act;
  h->Wl.resize(h->L);
  for (int l = 0; l < h->L; ++l) TRY(alloc_tensor(h->Wl[l], l == 0 ? 2 * N + 1 : e + 1, e, true, 1));
  TRY(alloc_tensor(h->Wo, 1, e + 1, true, 1));      // (every CFGAN tensor owns its gradient buffer)
  h->Al.resize(h->L);
  std::vector<float> ones((size_t)2 * B, 1.0f);
  for (int l = 0; l < h->L; ++l) {
    TRY(h->Al[l].alloc((size_t)2 * B * h->lde, true));
    HIP_TRY(hipMemcpy2D(h->Al[l] + e, (size_t)h->lde * 4, ones.data(), 4, 4, (size_t)2 * B, hipMemcpyHostToDevice));
  }
  TRY(h->dz0.alloc((size_t)2 * B * h->lde, true));
  TRY(h->dz1.alloc((size_t)2 * B * h->lde, true));
  TRY(h->dlogit.alloc((size_t)2 * B, true));
  return 0;
}

// gW = A_ext^T . dz over `nrows` rows, TF-Adam in the epilogue (the plan DisGANMF's weight gradients run on)
int cfgan_wgrad(ganmf_handle* h, const float* A, int lda, const float* dz, int ldz, Tensor& W, int M, int N, int nrows, int alpha_idx, float reg) {
  GemmP g{};
  g.A = A; g.lda = lda; g.B = dz; g.ldb = ldz;
  g.C = W.g; g.ldc = W.ld; g.M = M; g.N = N; g.K = nrows;
  g.epi.kind = EPI_ADAM; g.epi.adam_theta = W.p; g.epi.adam_m = W.m; g.epi.adam_v = W.v;
  g.epi.adam_alpha = h->scal + alpha_idx; g.epi.adam_reg = reg;
  GemmTune ft;
  ft.tile = 64; ft.ring = 2; ft.nsplit = 1;
  ft.mode = h->tune.mode != MFMA_AUTO ? h->tune.mode : FUSED_MODE;
  ft.bk = FUSED_BK;
  return run_gemm(h, T_DIS_GW, T_RED_DIS_GW, g, true, true, nullptr, 24.0 * W.count(), 0, &ft);
}

// One optimiser step on rows [row0, row0 + nb): kind 0 the discriminator's, 1 the generator's.  The step's loss -> *loss_dev.
int cfgan_step(ganmf_handle* h, int kind, int row0, int nb, float* loss_dev) {
  CfganState& c = h->cf;
  const int N = h->N, e = h->e, L = h->L;
  const bool gstep = kind == 1;
  const int alpha = gstep ? S_ALPHA_G : S_ALPHA_D;
  const float reg = gstep ? h->cfg.g_reg : h->cfg.d_reg;
  const unsigned* pm = c.scheme != 0 ? c.planes + (size_t)CFGAN_PLANE_PM * h->U * c.words : nullptr;      // ZR: the train mask is c
  const unsigned* zr = (gstep && c.scheme != 1 && c.zr_coef != 0.f) ? c.planes + (size_t)CFGAN_PLANE_ZR * h->U * c.words : nullptr;
  std::vector<Tensor*> mine;
  if (gstep) mine = c.gen.tensors();
  else { for (auto& t : h->Wl) mine.push_back(&t); mine.push_back(&h->Wo); }
  GANMF_LAUNCH(open_step_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), kind, alpha, gstep ? h->cfg.g_lr : h->cfg.d_lr);
  HIP_TRY(hipGetLastError());
  if (reg != 0.f) TRY(sumsq_tensors(h, mine, c.sq));
  // rows, generator, masked rows into the discriminator's input block
  TRY(mlp_forward_rows(h, c.gen, nullptr, row0, nb, c.fake, h->ldN, c.C));
  CfganRowP rp{c.C, c.fake, c.dfake, h->ldN, N, nb, row0, pm, zr, c.words, c.DX, c.ldx, gstep ? 0 : 1, zr ? c.zr_part : nullptr,
               2.0f * c.zr_coef / (float)nb};
  GANMF_LAUNCH(cfgan_mask_fwd_kernel, dim3(nb), dim3(256), 0, h->st, rp);
  HIP_TRY(hipGetLastError());
  // discriminator forward over M rows, head, top of the backward pass
  const int M = gstep ? nb : 2 * nb;
  for (int l = 0; l < L; ++l) {
    GemmP q{};
    q.A = l == 0 ? c.DX : h->Al[l - 1]; q.lda = l == 0 ? c.ldx : h->lde;
    q.B = h->Wl[l].p; q.ldb = h->lde;
    q.C = h->Al[l]; q.ldc = h->lde; q.M = M; q.N = e; q.K = l == 0 ? 2 * N + 1 : e + 1;
    q.epi.kind = EPI_ACT; q.epi.act = h->act;
    TRY(run_gemm(h, T_DIS_FWD, T_RED_DIS_FWD, q, false, true));
  }
  float* feat = h->Al[L - 1];
  float* la = c.loss_rows;
  float* lb = c.loss_rows + c.Bm;
  // rows < nb carry label 1: the real half of a D-step, and ALL rows of a G-step (CFGAN.py:164: the generator wants its rows called real)
  GANMF_LAUNCH(dis_head_kernel, dim3((M + 3) / 4), dim3(256), 0, h->st, feat, h->lde, e + 1, h->Wo.p.get(), 0, M, nb, 1.0f / (float)nb, h->dlogit.get(), la, lb);
  HIP_TRY(hipGetLastError());
  GANMF_LAUNCH(cfgan_loss_kernel, dim3(1), dim3(256), 0, h->st, la, gstep ? (const float*)nullptr : lb, nb,
               reg != 0.f ? c.sq : (const float*)nullptr, (int)mine.size() * CFGAN_SQ_BLOCKS, reg, zr ? c.zr_part : (const float*)nullptr, c.zr_coef, loss_dev);
  HIP_TRY(hipGetLastError());
  GANMF_LAUNCH(dis_dz_top_kernel, dim3(dis_dz_top_blocks(e)), dim3(DZ_COLS * DZ_GROUPS), 0, h->st, feat, h->lde, e, h->Wo.p.get(), h->dlogit.get(),
               0, M, 0, 0.f, h->act, h->dz0.get(), (float*)nullptr, (float*)nullptr, gstep ? (float*)nullptr : h->Wo.p, h->Wo.m.get(), h->Wo.v.get(),
               h->scal.get(), alpha, reg, (float*)nullptr, (const float*)nullptr, 0, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  HIP_TRY(hipGetLastError());
  // hidden layers, top down: the product that reads W_l (backward) in front of the one that updates it
  float* cur = h->dz0;
  float* nxt = h->dz1;
  for (int l = L - 1; l >= 0; --l) {
    if (l > 0) TRY(mlp_bwd(h, cur, h->lde, h->Wl[l].p, h->lde, nxt, h->lde, M, e, e, h->act, h->Al[l - 1], h->lde));
    if (!gstep) TRY(cfgan_wgrad(h, l == 0 ? c.DX : h->Al[l - 1], l == 0 ? c.ldx : h->lde, cur, h->lde, h->Wl[l], l == 0 ? 2 * N + 1 : e + 1, e, M, alpha, reg));
    if (l > 0) std::swap(cur, nxt);
  }
  if (!gstep) return 0;
  // d loss / d g_out = dz_0 . W_0[N:2N]^T, then dfake through the masks
  TRY(mlp_bwd(h, cur, h->lde, h->Wl[0].p + (size_t)N * h->lde, h->lde, c.dfake, h->ldN, nb, N, e, 0, nullptr, 0));
  GANMF_LAUNCH(cfgan_mask_bwd_kernel, dim3(nb), dim3(256), 0, h->st, rp);
  HIP_TRY(hipGetLastError());
  return mlp_backward(h, c.gen, c.C, c.dfake, c.dh0, c.dh1, nb, [&](const float* A, int lda, const float* dz, int ldz, Tensor& W, int Mw, int Nw) {
    return cfgan_wgrad(h, A, lda, dz, ldz, W, Mw, Nw, nb, alpha, reg);
  });
}

// The third score source behind scores_device.  transposed = 0: out[i, :] = G(c[ids[i]]) (user mode).  transposed = 1: row ids[i] of the
// TRANSPOSED G(all rows) (item mode: training rows are items), formed in blocks into a device cache keyed by param_version.
int cfgan_scores(ganmf_handle* h, const int* ids_dev, int64_t n, int transposed, float* out, int ldw) {
  CfganState& c = h->cf;
  if (!c.ready) return fail(-1, "scores: ganmf_cfgan_init has not been called on this GANMF_MODEL_CFGAN handle");
  if (!h->has_urm) return fail(-1, "scores: ganmf_set_urm_csr has not been called");
  const int N = h->N, U = h->U;
  if (!transposed) return mlp_forward_rows(h, c.gen, ids_dev, 0, (int)n, out, ldw);
  const int ldu = round_up(U, LD_ALIGN);      // == ldw
  if (c.cache_version != h->param_version || !c.cache) {
    if (!c.cache) TRY(c.cache.alloc((size_t)N * ldu, true));
    const int blk = std::min(U, 1024);
    TRY(mlp_scratch(h, c.gen, (size_t)blk));      // grown here: sc_F is named as the output below, before mlp_forward_rows would grow it
    for (int r0 = 0; r0 < U; r0 += blk) {
      const int nb = std::min(blk, U - r0);
      TRY(mlp_forward_rows(h, c.gen, nullptr, r0, nb, c.gen.sc_F, h->ldN));
      GANMF_LAUNCH(cfgan_transpose_kernel, dim3((N + 31) / 32, (nb + 31) / 32), dim3(256), 0, h->st, c.gen.sc_F.get(), h->ldN, nb, N, c.cache.get(), ldu, r0);
      HIP_TRY(hipGetLastError());
    }
    c.cache_version = h->param_version;
  }
  const long long total = (long long)n * (ldu / 4);
  GANMF_LAUNCH(gather_rows_kernel, dim3((int)std::min<long long>(2048, (total + 255) / 256)), dim3(256), 0, h->st, c.cache.get(), ldu, ids_dev, (int)n, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

