// abi_als.inc -- C ABI: implicit-feedback ALS (WRMF) on the factor tensors: ganmf_als_set_confidence / ganmf_als_half_sweep
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
int ganmf_als_set_confidence(ganmf_handle* h, int side, const int64_t* indptr, const int32_t* indices, const float* conf,
                             int64_t n_rows, int64_t n_cols) {
  const char* who = "ganmf_als_set_confidence";
  if (!h || !indptr) return fail(-1, "%s: null argument", who);
  if (side != 0 && side != 1) return fail(-1, "%s: side must be 0 (users x items) or 1 (items x users)", who);
  const int64_t want_r = side == 0 ? h->U : h->N, want_c = side == 0 ? h->N : h->U;
  if (n_rows != want_r || n_cols != want_c)
    return fail(-1, "%s: side %d is %lld x %lld on this handle, given %lld x %lld", who, side, (long long)want_r, (long long)want_c,
                (long long)n_rows, (long long)n_cols);
  TRY(check_csr(who, indptr, indices, n_rows, n_cols, false, false));
  const int64_t nnz = indptr[n_rows];
  if (nnz > 0 && !conf) return fail(-1, "%s: null argument", who);
  for (int64_t j = 0; j < nnz; ++j)
    if (!std::isfinite(conf[j])) return fail(-1, "%s: confidence %lld is not finite", who, (long long)j);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  AlsSide& s = h->als[side];
  s.canonical = false; s.conf.reset();
  TRY(s.upload(indptr, indices, n_rows, n_cols));
  TRY(s.upload_values(s.conf, conf));
  s.canonical = true;
  for (int64_t r = 0; r < n_rows && s.canonical; ++r)
    for (int64_t j = indptr[r] + 1; j < indptr[r + 1]; ++j)
      if (indices[j] <= indices[j - 1]) { s.canonical = false; break; }
  return 0;
}

int ganmf_als_half_sweep(ganmf_handle* h, int side, float reg) {
  const char* who = "ganmf_als_half_sweep";
  if (!h) return fail(-1, "null handle");
  TRY(needs_tensors(h, who));
  TRY(not_cfgan(h, who));
  if (side != 0 && side != 1) return fail(-1, "%s: side must be 0 (user factors from item factors) or 1 (the reverse)", who);
  const int k = h->k;
  if (k > ALS_MAX_K) return fail(-1, "%s: num_factors %d is above the limit of %d (a row's packed triangle has to fit the LDS of a CU)", who, k, ALS_MAX_K);
  if (h->has_comm && h->cfg.world_size > 1) return fail(-1, "%s: single-GPU entry", who);
  const AlsSide& s = h->als[side];
  if (!s.indptr) return fail(-1, "%s: ganmf_als_set_confidence has not been called for side %d", who, side);
  if (!std::isfinite(reg)) return fail(-1, "%s: reg is not finite", who);
  HIP_TRY(hipSetDevice(h->dev));
  Tensor& Yt = side == 0 ? h->V : h->Ue;      // held fixed
  Tensor& Xt = side == 0 ? h->Ue : h->V;      // solved
  const int n_fixed = Yt.rows, n_rows = Xt.rows, ld = h->ldk;
  if (!h->als_G) TRY(h->als_G.alloc((size_t)ld * ld, true));
  if (!h->als_bad) TRY(h->als_bad.alloc((size_t)std::max(h->U, h->N) + 1, true));
  ++h->param_version;
  {      // G = Y^T Y on the fp32 MFMA whatever the handle's training arithmetic is (split along K by the planner)
    GemmP g{};
    g.A = Yt.p; g.lda = ld; g.B = Yt.p; g.ldb = ld; g.C = h->als_G; g.ldc = ld;
    g.M = k; g.N = k; g.K = n_fixed; g.epi.kind = EPI_STORE;
    GemmTune ft;
    ft.mode = MFMA_F32;
    TRY(run_gemm(h, T_GEMM_GV, T_RED_GV, g, true, true, nullptr, 0, 0, &ft));
  }
  HIP_TRY(hipMemsetAsync(h->als_bad, 0, ((size_t)n_rows + 1) * sizeof(int), h->st));
  AlsP p{};
  p.Y = Yt.p; p.G = h->als_G; p.X = Xt.p; p.ldy = ld; p.ldg = ld; p.ldx = ld;
  p.indptr = s.indptr; p.indices = s.indices; p.conf = s.conf;
  p.n_rows = n_rows; p.k = k; p.reg = reg; p.bad = h->als_bad;
  if (k <= 32) {
    GANMF_LAUNCH(als_rows_small_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(ALS_THREADS), 0, h->st, p);
  } else {
    const int nt = (k + 31) / 32, need = (nt * (nt + 1) / 2 + 3) / 4;
    const size_t shmem = als_lds_floats(k) * sizeof(float);
    if (need <= 1) {
      TRY(allow_lds((const void*)als_rows_mfma_kernel<1>, shmem));
      GANMF_LAUNCH(als_rows_mfma_kernel<1>, dim3((unsigned)n_rows), dim3(ALS_THREADS), shmem, h->st, p);
    } else if (need <= 3) {
      TRY(allow_lds((const void*)als_rows_mfma_kernel<3>, shmem));
      GANMF_LAUNCH(als_rows_mfma_kernel<3>, dim3((unsigned)n_rows), dim3(ALS_THREADS), shmem, h->st, p);
    } else if (need <= 6) {
      TRY(allow_lds((const void*)als_rows_mfma_kernel<6>, shmem));
      GANMF_LAUNCH(als_rows_mfma_kernel<6>, dim3((unsigned)n_rows), dim3(ALS_THREADS), shmem, h->st, p);
    } else {
      TRY(allow_lds((const void*)als_rows_mfma_kernel<9>, shmem));
      GANMF_LAUNCH(als_rows_mfma_kernel<9>, dim3((unsigned)n_rows), dim3(ALS_THREADS), shmem, h->st, p);
    }
  }
  HIP_TRY(hipGetLastError());
  int any = 0;
  HIP_TRY(hipMemcpyAsync(&any, h->als_bad, sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (any) {
    std::vector<int> bad((size_t)n_rows);
    HIP_TRY(hipMemcpy(bad.data(), h->als_bad + 1, bad.size() * sizeof(int), hipMemcpyDeviceToHost));
    const int64_t first = std::find(bad.begin(), bad.end(), 1) - bad.begin();
    return fail(-4, "%s: side %d, row %lld: the system B = Y^T Y + sum (c - 1) y y^T + reg I is not positive definite (reg = %g); "
                    "the rows with such a system keep their factors", who, side, (long long)first, (double)reg);
  }
  return 0;
}
