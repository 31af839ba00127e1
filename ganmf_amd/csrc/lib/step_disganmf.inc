// step_disganmf.inc -- DisGANMF: forward, backward and the two updates (DisGANMF.py:57-79,110-140)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// =================================================================================================
// DisGANMF (GANRec/DisGANMF.py:57-79,110-140): binary MLP discriminator on [float(uid) | profile].
// Layer-0 input = XF with the ones column at N and float(uid) at column N+1; W_0_ext rows follow the
// same order (profile rows, bias row, uid row), so the uid term is an exact fp32 rank-1 part of the
// same GEMM.  Hidden outputs carry a ones column at e (bias folding as in GANMF).
// =================================================================================================
// head != nullptr: the caller wants logits / cross-entropies / dlogit of rows [head->row0, head->row0 + head->nrows) of the last
// layer's output.  *head_done = true when they were formed by the last layer's slab-sum launch (reduce_rows_head_kernel: the
// forward GEMM was split along K and had a reduce launch anyway); else the caller launches dis_head_kernel.
int dis_forward(ganmf_handle* h, const int* rows_dev, int nb, int which, const HeadP* head = nullptr, bool* head_done = nullptr) {
  if (head_done) *head_done = false;
  const int N = h->N, k = h->k, e = h->e;
  // X rows with the float(uid) column, Ub, F = Ub . V^T   (DisGANMF.py:59,77-78)
  TRY(rows_and_generator(h, rows_dev, nb, which, which ? h->g_alpha : h->d_alpha, N + 1, (int)h->cfg.row_offset));
  (void)k;
  for (int l = 0; l < h->L; ++l) {  // a_l = act([a_{l-1} | 1 (| uid)] . W_l_ext)   (DisGANMF.py:60-62)
    GemmP g{};
    g.A = l == 0 ? h->XF : h->Al[l - 1]; g.lda = l == 0 ? h->ldN : h->lde;
    g.B = h->Wl[l].p; g.ldb = h->lde;
    g.C = h->Al[l]; g.ldc = h->lde; g.M = 2 * nb; g.N = e; g.K = l == 0 ? N + 2 : e + 1;
    g.epi.kind = EPI_ACT; g.epi.act = h->act;
    if (l == 0 && low_precision(h)) {
      // float(uid) (up to 6039: not representable in 8 or 11 bits) stays fp32: column N+1 of the input leaves the K range
      // and comes back as a rank-1 term of the epilogue, uid[m] * W_0_ext[N+1, n]
      g.K = N + 1;
      g.epi.r1_u = h->XF + (N + 1); g.epi.r1_ld = h->ldN;
      g.epi.r1_w = h->Wl[0].p + (size_t)(N + 1) * h->lde;
    }
    if (l == h->L - 1 && head && head_done && (h->multi & 1) && tune_env_int("dis_head_fuse", 1)) {      // (GANMF_MULTI bit 0 off: one kernel per piece)
      RedP red{};
      TRY(run_gemm(h, T_DIS_FWD, T_RED_DIS_FWD, g, false, true, nullptr, 0, 0, nullptr, nullptr, &red));
      if (red.part) {      // split: its reduce is ours to launch -- with the head riding in it
        Scope s(h, T_RED_DIS_FWD, 0, 4.0 * (red.nsplit + 1) * red.M * red.N);
        GANMF_LAUNCH(reduce_rows_head_kernel, dim3(red.M), dim3(256), 0, h->st, red, *head);
        HIP_TRY(hipGetLastError());
        *head_done = true;
      }
      continue;
    }
    TRY(run_gemm(h, T_DIS_FWD, T_RED_DIS_FWD, g, false, true));
  }
  return 0;
}

// dz_{l-1} = (dz_l . W_l[0:e]^T) * act'(a_{l-1}) for rows [row0, row0+nrows); returns the dz_0 buffer
int dis_backprop_hidden(ganmf_handle* h, int row0, int nrows, bool param_grads, int b_global, float** dz0_out) {
  const float gsc = grad_scale(h, b_global);     // dz carries the 1/B of the mean cross-entropy times an output weight
  const int N = h->N, e = h->e;
  float* cur = h->dz0;   // dz_{L-1} was written here by dis_dz_top_kernel
  float* nxt = h->dz1;
  auto backward = [&](int l) -> int {      // dz_{l-1} = (dz_l . W_l[0:e]^T) * act'(a_{l-1}): cur -> nxt
    GemmP g{};
    g.A = cur + (size_t)row0 * h->lde; g.lda = h->lde; g.B = h->Wl[l].p; g.ldb = h->lde;
    g.C = nxt + (size_t)row0 * h->lde; g.ldc = h->lde; g.M = nrows; g.N = e; g.K = e;
    g.epi.kind = EPI_MUL_ACTGRAD; g.epi.act = h->act;
    g.epi.aux = h->Al[l - 1] + (size_t)row0 * h->lde; g.epi.ldaux = h->lde;
    g.a_scale = gsc;
    return run_gemm(h, T_DIS_BWD, T_RED_DIS_BWD, g, false, false);
  };
  for (int l = h->L - 1; l >= 0; --l) {
    if (param_grads) {  // gW_l_ext = [a_{l-1} | 1 (| uid)]^T . dz_l  (all 2B rows: row0 = 0)
      GemmP g{};
      g.A = l == 0 ? h->XF : h->Al[l - 1]; g.lda = l == 0 ? h->ldN : h->lde;
      g.B = cur; g.ldb = h->lde;
      g.C = h->Wl[l].g; g.ldc = h->lde; g.M = l == 0 ? N + 2 : e + 1; g.N = e; g.K = nrows;
      g.epi.kind = EPI_STORE;
      g.b_scale = gsc;
      const bool uid_apart = l == 0 && low_precision(h);
      if (uid_apart) g.M = N + 1;      // the float(uid) row of W_0_ext gets its gradient from the fp32 reduction below
      // TF-Adam runs in the epilogue of the gradient GEMM, as for GANMF's two tensors -- the gradient is never stored, no
      // adam_dense pass.  Layer 0 holds nearly all discriminator parameters ([N+2, e]) and nothing reads W_0 after its gradient
      // in this step; a hidden layer's W_l is read once more, by the backward product dz_{l-1} = dz_l . W_l^T, which therefore
      // goes FIRST (below).  Not with a communicator (the gradient must be reduced first).  In the low-precision modes the
      // float(uid) row of layer 0 is left out of the GEMM and updated by the fp32 kernel below.
      const bool fuse = !h->has_comm && (l == 0 || h->dis_fuse_hidden);
      h->dis_fused[l] = 0;
      if (l > 0 && fuse) TRY(backward(l));
      if (fuse) {
        const bool regD = h->cfg.d_reg != 0.f;
        g.epi.kind = EPI_ADAM; g.epi.adam_theta = h->Wl[l].p; g.epi.adam_m = h->Wl[l].m; g.epi.adam_v = h->Wl[l].v;
        g.epi.adam_alpha = h->scal + h->d_alpha; g.epi.adam_reg = h->cfg.d_reg;
        g.epi.sq_partials = regD ? h->dis_slot + (size_t)(4 + l) * h->dis_cap : nullptr;
        GemmTune ft;
        ft.tile = 64; ft.ring = 2; ft.nsplit = 1;
        ft.mode = h->tune.mode != MFMA_AUTO ? h->tune.mode : FUSED_MODE;
        ft.bk = FUSED_BK;
        int regn = ADAM_GRID;
        if (l == 0 && h->dis_colsum_pending) {
          // the column sums of the top of the backward pass (output-layer gradient + Adam, the fp32 float(uid) row) as extra blocks of this
          // launch: gemm_bf16s_colsum (the plan was checked by dis_d_step: the staged 64 x 64 kernel, unsplit)
          h->dis_colsum_pending = false;
          g.nbatch = 1; g.zero_page = h->zero_page;
          g.n_fastest = 1;
          const GemmPlan pl = gemm_plan(g.M, g.N, g.K, 1, g.epi.sq_partials != nullptr, ft, true);
          fill_plan(g, pl);
          regn = pl.sq_count;
          const int ng = pl.tiles_m * pl.tiles_n, ncs = dis_colsum_blocks(e);
          Scope s(h, T_DIS_GW, gemm_flops(g.M, g.N, g.K), gemm_bytes(g.M, g.N, g.K) + 24.0 * h->Wl[l].count());
          if (pl.mode == MFMA_F16) GANMF_LAUNCH((gemm_bf16s_colsum<64, 1, true>), dim3(ng + ncs), dim3(256), 0, h->st, g, h->dis_colsum, ncs);
          else if (pl.mode == MFMA_BF16) GANMF_LAUNCH((gemm_bf16s_colsum<64, 1, false>), dim3(ng + ncs), dim3(256), 0, h->st, g, h->dis_colsum, ncs);
          else GANMF_LAUNCH((gemm_bf16s_colsum<32, 3, false>), dim3(ng + ncs), dim3(256), 0, h->st, g, h->dis_colsum, ncs);
          HIP_TRY(hipGetLastError());
        } else
        TRY(run_gemm(h, T_DIS_GW, T_RED_DIS_GW, g, true, true, &regn, 24.0 * h->Wl[l].count(), 0, &ft));
        h->dis_fused[l] = 1;
        h->dis_regn[l] = regn;
        if (l > 0) { std::swap(cur, nxt); continue; }      // (the backward product of this layer is done)
      } else
      TRY(run_gemm(h, T_DIS_GW, T_RED_DIS_GW, g, true, true));
      if (uid_apart && !h->dis_uid_done) {      // (else: gradient + update of the float(uid) row rode in dis_dz_top_kernel, dis_d_step)
        const size_t ro = (size_t)(N + 1) * h->lde;      // the float(uid) row of W_0_ext
        const int nblk = (e + 63) / 64;
        const bool apply = h->dis_fused[0] && h->dis_regn[0] + nblk <= h->dis_cap;
        if (h->dis_fused[0] && !apply) return fail(-1, "dis_backprop_hidden: no room for the uid row's sum(theta^2) partials");
        const bool regD = h->cfg.d_reg != 0.f;
        GANMF_LAUNCH(dis_uid_grad_kernel, dim3(nblk), dim3(64 * UIDG_GROUPS), 0, h->st, h->XF, h->ldN, N + 1, cur, h->lde,
                           nrows, e, h->Wl[0].g + ro, apply ? h->Wl[0].p + ro : nullptr, h->Wl[0].m + ro, h->Wl[0].v + ro,
                           h->scal.get(), h->d_alpha, h->cfg.d_reg,
                           (apply && regD) ? h->dis_slot + (size_t)4 * h->dis_cap + h->dis_regn[0] : nullptr);
        HIP_TRY(hipGetLastError());
        if (apply && regD) h->dis_regn[0] += nblk;
      }
    }
    if (l > 0) {
      TRY(backward(l));
      std::swap(cur, nxt);
    }
  }
  *dz0_out = cur;
  return 0;
}

int dis_d_step(ganmf_handle* h, const int* rows_dev, int nb, int b_global, float* parts) {
  const int e = h->e;
  const float inv_b = 1.0f / (float)b_global;
  const bool fuse_wo = !h->has_comm && h->dis_fuse_hidden;      // output layer updated by the kernel that forms its gradient
  h->dis_colsum_pending = false;
  h->dis_uid_done = false;
  if (nb > 0) {
    // One layer, fused Adam, single GPU (round 6): the row-local part of the top of the backward pass (dz_0) is written by the workgroup that
    // sums the row's slabs and forms its logit (reduce_rows_head_kernel, HeadP::dz_rows); the column sums -- output-layer gradient + Adam, and in
    // the low-precision modes the fp32 float(uid) row of W_0_ext -- ride in the layer-0 gradient GEMM's launch (gemm_bf16s_colsum):
    // dis_dz_top_kernel and dis_uid_grad_kernel leave the step.  Only when that GEMM is planned onto the staged 64 x 64 kernel, unsplit, and
    // the head does ride in the slab sum (else the kernels of rounds 2-5).  GANMF_TUNE dis_top_gw=0 keeps those.
    bool top_gw = h->L == 1 && fuse_wo && (h->multi & 1) && tune_env_int("dis_top_gw", 1) != 0;
    if (top_gw) {
      GemmTune ft;
      ft.tile = 64; ft.ring = 2; ft.nsplit = 1;
      ft.mode = h->tune.mode != MFMA_AUTO ? h->tune.mode : FUSED_MODE;
      ft.bk = FUSED_BK;
      const GemmPlan pl = gemm_plan(low_precision(h) ? h->N + 1 : h->N + 2, e, 2 * nb, 1, h->cfg.d_reg != 0.f, ft, true);
      top_gw = pl.tile == 64 && pl.nsplit == 1 && !pl.persist &&
               ((pl.mode == MFMA_BF16X3 && pl.bk == 32) || pl.mode == MFMA_F16 || pl.mode == MFMA_BF16) &&
               2 * dis_colsum_blocks(e) <= h->dis_cap;
    }
    HeadP head{h->Wo.p, 0, 2 * nb, nb, inv_b, h->dlogit, h->dis_slot, h->dis_slot + h->dis_cap, 0, 0.f, h->act, nullptr, nullptr};
    if (top_gw) { head.dz = h->dz0; head.dz_rows = 1; }
    bool head_done = false;
    TRY(dis_forward(h, rows_dev, nb, 0, &head, &head_done));
    float* feat = h->Al[h->L - 1];
    if (top_gw && head_done) {
      const bool regD = h->cfg.d_reg != 0.f;
      const int ncs = dis_colsum_blocks(e);
      const bool lp = low_precision(h);
      const size_t ro = (size_t)(h->N + 1) * h->lde;      // the float(uid) row of W_0_ext
      float* const seg = h->dis_slot + (size_t)(4 + h->L) * h->dis_cap;      // (finish_dis_parts_kernel sums whole segments)
      h->dis_colsum = ColSumP{feat, h->lde, e, h->dlogit, 2 * nb, h->dz0, h->Wo.p, h->Wo.m, h->Wo.v, h->scal, h->d_alpha, h->cfg.d_reg,
                              regD ? seg : nullptr, lp ? (const float*)(h->XF + (h->N + 1)) : nullptr, h->ldN,
                              lp ? h->Wl[0].p + ro : nullptr, lp ? h->Wl[0].m + ro : nullptr, lp ? h->Wl[0].v + ro : nullptr,
                              (lp && regD) ? seg + ncs : nullptr};
      h->dis_colsum_pending = true;
      h->dis_uid_done = lp;
    } else {
    // One layer, low-precision K loops, fused Adam: the top of the backward pass writes dz_0 itself, so the fp32 float(uid) row of W_0_ext
    // gets its gradient and its TF-Adam update in that launch (dis_uid_grad_kernel's launch leaves the step; GANMF_TUNE dis_uid_top=0 keeps it).
    // Its sum(theta^2) partials go behind the output layer's in the same arena segment (finish_dis_parts_kernel sums whole segments).
    const int ntop = dis_dz_top_blocks(e);
    const bool uid_top = h->L == 1 && low_precision(h) && !h->has_comm && 2 * ntop <= h->dis_cap && tune_env_int("dis_uid_top", 1);
    h->dis_uid_done = uid_top;
    {
      Scope s(h, T_DIS_HEAD, 0, 4.0 * 2 * nb * e * 3);
      if (!head_done)
      GANMF_LAUNCH(dis_head_kernel, dim3((2 * nb + 3) / 4), dim3(256), 0, h->st, feat, h->lde, e + 1,
                         h->Wo.p.get(), 0, 2 * nb, nb, inv_b, h->dlogit.get(), h->dis_slot, h->dis_slot + h->dis_cap);
      const size_t ro = (size_t)(h->N + 1) * h->lde;      // the float(uid) row of W_0_ext
      GANMF_LAUNCH(dis_dz_top_kernel, dim3(ntop), dim3(DZ_COLS * DZ_GROUPS), 0, h->st, feat, h->lde, e,
                         h->Wo.p.get(), h->dlogit.get(), 0, 2 * nb, 0, 0.f, h->act, h->dz0.get(), h->Wo.g, (float*)nullptr,
                         fuse_wo ? h->Wo.p : nullptr, h->Wo.m.get(), h->Wo.v.get(), h->scal.get(), h->d_alpha, h->cfg.d_reg,
                         (fuse_wo && h->cfg.d_reg != 0.f) ? h->dis_slot + (size_t)(4 + h->L) * h->dis_cap : nullptr,
                         uid_top ? (const float*)(h->XF + (h->N + 1)) : (const float*)nullptr, h->ldN,
                         uid_top ? h->Wl[0].p + ro : (float*)nullptr, uid_top ? h->Wl[0].m + ro : (float*)nullptr,
                         uid_top ? h->Wl[0].v + ro : (float*)nullptr,
                         (uid_top && h->cfg.d_reg != 0.f) ? h->dis_slot + (size_t)(4 + h->L) * h->dis_cap + ntop : (float*)nullptr);
      HIP_TRY(hipGetLastError());
    }
    }
    float* dz0;
    TRY(dis_backprop_hidden(h, 0, 2 * nb, true, b_global, &dz0));
    if (h->dis_colsum_pending) return fail(-1, "dis_d_step: the column sums of the backward top were not launched");
  } else {
    GANMF_LAUNCH(open_step_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), 0, h->d_alpha, h->cfg.d_lr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(h->gD, 0, h->gD_elems * sizeof(float), h->st));
  }
  const bool reg = h->cfg.d_reg != 0.f;
  if (h->has_comm) {
    for (int l = 0; l < h->L; ++l)
      TRY(dp_update(h, T_ADAM_D, h->Wl[l], h->d_alpha, h->cfg.d_reg, reg ? h->dis_slot + (size_t)(4 + l) * h->dis_cap : nullptr, 0));
    TRY(dp_update(h, T_ADAM_D, h->Wo, h->d_alpha, h->cfg.d_reg, reg ? h->dis_slot + (size_t)(4 + h->L) * h->dis_cap : nullptr, 0));
  } else {
    for (int l = 0; l < h->L; ++l) {
      if (nb > 0 && h->dis_fused[l]) continue;      // updated in the epilogue of its gradient GEMM
      TRY(adam_dense(h, T_ADAM_D, h->Wl[l], h->Wl[l].g, h->d_alpha, h->cfg.d_reg, reg ? h->dis_slot + (size_t)(4 + l) * h->dis_cap : nullptr));
    }
    if (!(nb > 0 && fuse_wo))      // (else: updated by dis_dz_top_kernel, which forms its gradient)
      TRY(adam_dense(h, T_ADAM_D, h->Wo, h->Wo.g, h->d_alpha, h->cfg.d_reg, reg ? h->dis_slot + (size_t)(4 + h->L) * h->dis_cap : nullptr));
  }
  // parts = {sum sce(real), sum sce(fake), sum theta_D^2}: summed from the slot once per epoch (arenas_finish)
  (void)parts; (void)reg;
  return 0;
}

int dis_g_step(ganmf_handle* h, const int* rows_dev, int nb, int start, int b_global, float* parts) {
  const int N = h->N, e = h->e;
  const float alpha = h->cfg.recon_coefficient;
  const float inv_b = 1.0f / (float)b_global;
  int fmn = 0;
  if (nb > 0) {
    const float fmc = alpha * 2.0f / ((float)b_global * (float)e);
    // generated rows only -> seg 0; with the head inside the slab-sum launch the top of the backward pass rides there too (row pairs)
    const HeadP head{h->Wo.p, nb, nb, nb, inv_b, h->dlogit, nullptr, h->dis_slot, nb <= h->dis_cap ? nb : 0, fmc, h->act, h->dz0,
                     h->dis_slot + h->dis_cap};
    bool head_done = false;
    TRY(dis_forward(h, rows_dev, nb, 1, &head, &head_done));
    float* feat = h->Al[h->L - 1];
    {  // generator loss = loss_fake + alpha * FM  (DisGANMF.py:135-136): generated rows only, label 0
      Scope s(h, T_DIS_HEAD, 0, 4.0 * 2 * nb * e * 3);
      if (!head_done)
      GANMF_LAUNCH(dis_head_kernel, dim3((nb + 3) / 4), dim3(256), 0, h->st, feat, h->lde, e + 1, h->Wo.p.get(),
                         nb, nb, nb, inv_b, h->dlogit.get(), (float*)nullptr, h->dis_slot);      // generated rows only -> seg 0
      fmn = (head_done && head.pair_off > 0) ? nb : dis_dz_top_blocks(e);
      if (!(head_done && head.pair_off > 0))
      GANMF_LAUNCH(dis_dz_top_kernel, dim3(fmn), dim3(DZ_COLS * DZ_GROUPS), 0, h->st, feat, h->lde, e, h->Wo.p.get(), h->dlogit.get(),
                         nb, nb, nb, fmc, h->act, h->dz0.get(), (float*)nullptr, h->dis_slot + h->dis_cap, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                         h->scal.get(), 0, 0.f, (float*)nullptr, (const float*)nullptr, 0, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
      HIP_TRY(hipGetLastError());
    }
    float* dz0;
    TRY(dis_backprop_hidden(h, nb, nb, false, b_global, &dz0));
    {  // dF = dz_0 . W_0[profile rows]^T     (the uid column of the input is dropped, DisGANMF.py:59)
      GemmP g{};
      g.A = dz0 + (size_t)nb * h->lde; g.lda = h->lde; g.B = h->Wl[0].p; g.ldb = h->lde;
      g.C = h->dF; g.ldc = h->ldN; g.M = nb; g.N = N; g.K = e; g.epi.kind = EPI_STORE;
      g.a_scale = grad_scale(h, b_global);
      TRY(run_gemm(h, T_GEMM_DF, T_RED_DF, g, false, false));
    }
  } else {
    if (!h->lazy_pass) GANMF_LAUNCH(open_step_kernel, dim3(1), dim3(64), 0, h->st, h->scal.get(), 1, h->g_alpha, h->cfg.g_lr);
    HIP_TRY(hipGetLastError());
  }
  const bool reg = h->cfg.g_reg != 0.f;
  int regn_v = ADAM_GRID;
  TRY(gen_update(h, nb, start, b_global, &regn_v, h->dis_slot + (size_t)2 * h->dis_cap, h->dis_slot + (size_t)3 * h->dis_cap));
  // parts = {sum sce(fake), sum (feat_f - feat_r)^2, sum U^2, sum V^2}: summed from the slot once per epoch (arenas_finish)
  (void)parts; (void)reg; (void)fmn;
  return 0;
}

