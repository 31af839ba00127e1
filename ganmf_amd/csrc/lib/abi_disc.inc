// abi_disc.inc -- C ABI: discriminator inference on an arbitrary row list (disc_rows.hpp)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

int ganmf_set_discriminate_block(ganmf_handle* h, int64_t rows) {
  if (!h) return fail(-1, "null handle");
  if (rows < 0) return fail(-1, "ganmf_set_discriminate_block: %lld rows", (long long)rows);
  h->disc_block = rows;
  return 0;
}

// The arithmetic of every product of the call: the fp32-accurate plan of its shape (MFMA_AUTO: the exact three-way bf16 split or the
// fp32 MFMA), whatever mode the handle trains in, on the compiler-scheduled kernels, one tile per workgroup.
static GemmTune disc_tune() {
  GemmTune t;
  t.mode = MFMA_AUTO;
  t.persist = 0;
  return t;
}

// One block of ganmf_discriminate: rows ids_dev[0 .. nb) -> features in *feat_out ([nb, lde], columns 0 .. e), values in h->dr_val.
static int discriminate_block(ganmf_handle* h, const int* ids_dev, int nb, int generated, bool want_value, const float** feat_out) {
  const int N = h->N, e = h->e;
  const bool dis = h->cfg.model == GANMF_MODEL_DISGANMF;
  const GemmTune ft = disc_tune();
  const int cols_grid = (nb + 255) / 256;
  if (generated) {      // X[b, :] = U[ids[b]] . V^T, unfiltered (GANMF.py:82-83)
    const long long total = (long long)nb * (h->ldk / 4);
    GANMF_LAUNCH(gather_rows_kernel, dim3((int)std::min<long long>(2048, (total + 255) / 256)), dim3(256), 0, h->st, h->Ue.p.get(), h->ldk,
                 ids_dev, nb, h->dr_Ub.get());
    HIP_TRY(hipGetLastError());
    GemmP g{};
    g.A = h->dr_Ub; g.lda = h->ldk; g.B = h->V.p; g.ldb = h->ldk;
    g.C = h->dr_X; g.ldc = h->ldN; g.M = nb; g.N = N; g.K = h->k; g.epi.kind = EPI_STORE;
    TRY(run_gemm(h, T_GEMM_GEN, T_RED_GEN, g, false, false, nullptr, 0, 0, &ft));
  } else if (dis) {     // DisGANMF feeds the rows themselves to its layers: the block is expanded on the device
    Scope s(h, T_DENSIFY, 0, 4.0 * nb * h->ldN);
    GANMF_LAUNCH(disc_densify_kernel, dim3(nb), dim3(256), 0, h->st, h->urm.indptr.get(), h->urm.indices.get(), h->data.get(), ids_dev, h->dr_X.get(), h->ldN);
    HIP_TRY(hipGetLastError());
  }
  if (generated || dis) {      // the ones column of the input block and DisGANMF's float(uid) column
    GANMF_LAUNCH(disc_cols_kernel, dim3(cols_grid), dim3(256), 0, h->st, h->dr_X.get(), h->ldN, nb, N, dis ? N + 1 : -1, ids_dev,
                 (int)h->cfg.row_offset);
    HIP_TRY(hipGetLastError());
  }
  if (dis) {
    // a_l = act([a_{l-1} | 1 (| uid)] . W_l_ext) (DisGANMF.py:60-62), the step's layer products: float(uid) as the fp32 rank-1 term of
    // the layer-0 epilogue, outputs alternating between the two buffers
    float* out[2] = {h->dr_E, h->dr_A};
    for (int b = 0; b < 2; ++b) {
      GANMF_LAUNCH(disc_cols_kernel, dim3(cols_grid), dim3(256), 0, h->st, out[b], h->lde, nb, e, -1, ids_dev, 0);
      HIP_TRY(hipGetLastError());
    }
    const float* in = h->dr_X;
    for (int l = 0; l < h->L; ++l) {
      GemmP g{};
      g.A = in; g.lda = l == 0 ? h->ldN : h->lde; g.B = h->Wl[l].p; g.ldb = h->lde;
      g.C = out[l & 1]; g.ldc = h->lde; g.M = nb; g.N = e; g.K = l == 0 ? N + 1 : e + 1;
      g.epi.kind = EPI_ACT; g.epi.act = h->act;
      if (l == 0) {
        g.epi.r1_u = h->dr_X + (N + 1); g.epi.r1_ld = h->ldN;
        g.epi.r1_w = h->Wl[0].p + (size_t)(N + 1) * h->lde;
      }
      TRY(run_gemm(h, T_DIS_FWD, T_RED_DIS_FWD, g, false, true, nullptr, 0, 0, &ft));
      in = out[l & 1];
    }
    *feat_out = in;
    if (want_value) {      // logit = [a | 1] . wo_ext (DisGANMF.py:63)
      Scope s(h, T_DIS_HEAD, 2.0 * nb * (e + 1), 4.0 * nb * (e + 1));
      GANMF_LAUNCH(disc_logit_kernel, dim3((nb + 3) / 4), dim3(256), 0, h->st, in, h->lde, e + 1, h->Wo.p.get(), nb, h->dr_val.get());
      HIP_TRY(hipGetLastError());
    }
    return 0;
  }
  // GANMF: E = x . We + be (GANMF.py:64-65) -- a CSR row-sum for stored rows, the encode product for generated ones
  GANMF_LAUNCH(disc_cols_kernel, dim3(cols_grid), dim3(256), 0, h->st, h->dr_E.get(), h->lde, nb, e, -1, ids_dev, 0);
  HIP_TRY(hipGetLastError());
  if (!generated) {
    Scope s(h, T_DENSIFY, 0, 4.0 * nb * e + 4.0 * (double)h->urm.nnz / std::max(h->U, 1) * nb * e);
    GANMF_LAUNCH(csr_encode_rows_kernel, dim3(nb), dim3(256), 0, h->st, h->urm.indptr.get(), h->urm.indices.get(), h->data.get(), ids_dev, h->We.p.get(), h->lde, N, e,
                 h->dr_E.get());
    HIP_TRY(hipGetLastError());
  } else {
    GemmP g{};
    g.A = h->dr_X; g.lda = h->ldN; g.B = h->We.p; g.ldb = h->lde;
    g.C = h->dr_E; g.ldc = h->lde; g.M = nb; g.N = e; g.K = N + 1; g.epi.kind = EPI_STORE;
    TRY(run_gemm(h, T_GEMM_ENC, T_RED_ENC, g, false, true, nullptr, 0, 0, &ft));
  }
  *feat_out = h->dr_E;
  if (!want_value) return 0;
  {  // D(x) = mean_j (([E | 1] . Wd_ext)_j - x_j)^2 (GANMF.py:66-68 per row): the decode product, unsplit along K, never stored
    GemmP g{};
    g.A = h->dr_E; g.lda = h->lde; g.B = h->Wd.p; g.ldb = h->ldN;
    g.C = nullptr; g.ldc = h->ldN; g.M = nb; g.N = N; g.K = e + 1;
    g.zero_page = h->zero_page;
    g.nsplit = 1; g.k_per_split = round_up(g.K, GEMM_K_ALIGN); g.nbatch = 1;
    g.tiles_m = (nb + ROWSQ_TILE - 1) / ROWSQ_TILE; g.tiles_n = (N + ROWSQ_TILE - 1) / ROWSQ_TILE;
    g.epi.kind = EPI_SUB_AUX_SQ; g.epi.gram_partials = h->dr_part;
    if (generated) { g.epi.aux = h->dr_X; g.epi.ldaux = h->ldN; }
    else { g.epi.csr_indptr = h->urm.indptr; g.epi.csr_indices = h->urm.indices; g.epi.csr_data = h->data; g.epi.csr_rows = ids_dev; }
    {
      Scope s(h, T_GEMM_DEC, gemm_flops(g.M, g.N, g.K), 4.0 * ((double)nb * (e + 1) + (double)(e + 1) * N + (generated ? (double)nb * N : 0.0)));
      GANMF_LAUNCH(rowsq_bf16x3_kernel, dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(256), 0, h->st, g);
      HIP_TRY(hipGetLastError());
    }
    Scope s(h, T_RED_DEC, (double)nb * g.tiles_n, 8.0 * nb * (g.tiles_n + 1));
    GANMF_LAUNCH(rowsq_finish_kernel, dim3(cols_grid), dim3(256), 0, h->st, h->dr_part.get(), nb, g.tiles_n, N, h->dr_val.get());
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int ganmf_discriminate(ganmf_handle* h, const int32_t* rows, int64_t n, int generated, float* features, double* value) {
  const char* who = "ganmf_discriminate";
  if (!h) return fail(-1, "null handle");
  TRY(needs_tensors(h, who));
  TRY(not_cfgan(h, who));
  if (h->cfg.model == GANMF_MODEL_MF) return fail(-1, "%s: a GANMF_MODEL_MF handle has no discriminator", who);
  if (!features && !value) return fail(-1, "%s: neither features nor value asked for", who);
  if (n < 0 || n > (1 << 30)) return fail(-1, "%s: n out of range", who);
  if (n == 0) return 0;
  if (!rows) return fail(-1, "%s: null argument", who);
  for (int64_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= h->U) return fail(-1, "%s: row %d out of range [0,%d)", who, rows[i], h->U);
  if (!generated && !h->has_urm) return fail(-1, "%s: stored rows need ganmf_set_urm_csr", who);
  const bool dis = h->cfg.model == GANMF_MODEL_DISGANMF;
  const int N = h->N, e = h->e;
  const int tiles_n = (N + ROWSQ_TILE - 1) / ROWSQ_TILE;
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  // rows per block: what this call adds to the handle stays under a quarter of the free device memory (the rule of the pass buffers)
  const bool need_x = generated || dis;
  const size_t row_bytes = sizeof(float) * ((need_x ? (size_t)h->ldN : 0) + (generated ? (size_t)h->ldk : 0) + (size_t)h->lde * (dis ? 2 : 1)) +
                           sizeof(double) * ((dis ? 0 : (size_t)tiles_n) + 1);
  int64_t blk = n;
  if (h->disc_block > 0) blk = std::min(blk, h->disc_block);
  {
    const size_t have = sizeof(float) * ((need_x ? h->dr_X.cap : 0) + (generated ? h->dr_Ub.cap : 0) + h->dr_E.cap + (dis ? h->dr_A.cap : 0)) +
                        sizeof(double) * ((dis ? 0 : h->dr_part.cap) + h->dr_val.cap);
    if ((size_t)blk * row_bytes > have) {      // (buffers that already hold the block were admitted by an earlier call)
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(-2, "%s: hipMemGetInfo failed", who);
      const int64_t fit = (int64_t)(std::max(free_b / 4, have) / row_bytes);
      if (fit < 1) return fail(-1, "%s: one row needs %.1f MB, over a quarter of the %.1f MB free", who, row_bytes / 1048576.0, free_b / 1048576.0);
      blk = std::min(blk, fit);
    }
  }
  TRY(h->dr_ids.grow(h->st, (size_t)n, false));
  if (need_x) TRY(h->dr_X.grow(h->st, (size_t)blk * h->ldN, true));
  if (generated) TRY(h->dr_Ub.grow(h->st, (size_t)blk * h->ldk, true));
  TRY(h->dr_E.grow(h->st, (size_t)blk * h->lde, true));
  if (dis) TRY(h->dr_A.grow(h->st, (size_t)blk * h->lde, true));
  if (!dis && value) TRY(h->dr_part.grow(h->st, (size_t)blk * tiles_n, false));
  if (value) TRY(h->dr_val.grow(h->st, (size_t)blk, false));
  int rc = 0;
  hipError_t err = hipMemcpyAsync(h->dr_ids, rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->st);
  for (int64_t at = 0; at < n && rc == 0 && err == hipSuccess; at += blk) {
    const int nb = (int)std::min<int64_t>(blk, n - at);
    const float* feat = nullptr;
    rc = discriminate_block(h, h->dr_ids + at, nb, generated, value != nullptr, &feat);
    if (rc) break;
    if (features)
      err = hipMemcpy2DAsync(features + (size_t)at * e, (size_t)e * 4, feat, (size_t)h->lde * 4, (size_t)e * 4, (size_t)nb, hipMemcpyDeviceToHost, h->st);
    if (err == hipSuccess && value) err = hipMemcpyAsync(value + at, h->dr_val, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, h->st);
  }
  if (err == hipSuccess) err = hipStreamSynchronize(h->st);
  else hipStreamSynchronize(h->st);
  if (rc) return rc;
  if (err != hipSuccess) return fail(-2, "%s: %s", who, hipGetErrorString(err));
  return 0;
}
