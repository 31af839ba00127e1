// abi_svd.inc -- C ABI: PureSVD on the factor tensors: ganmf_pure_svd (randomized truncated SVD of the handle's weighted sparse matrix)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
constexpr int SVD_CODE_EIG = 1 << 20, SVD_CODE_SELECT = SVD_CODE_EIG + 1;

static int svd_ensure(ganmf_handle* h, int ldl) {
  const size_t rows = (size_t)std::max(h->U, h->N);
  if (h->svd_ldl >= ldl) return 0;
  HIP_TRY(hipStreamSynchronize(h->st));
  h->svd_P[0].reset(); h->svd_P[1].reset(); h->svd_G.reset(); h->svd_X.reset(); h->svd_Wl.reset(); h->svd_lam.reset(); h->svd_flag.reset();
  h->svd_ldl = 0;
  TRY(h->svd_P[0].alloc(rows * ldl, true));
  TRY(h->svd_P[1].alloc(rows * ldl, true));
  TRY(h->svd_G.alloc((size_t)ldl * ldl, true));
  TRY(h->svd_X.alloc((size_t)ldl * ldl, true));
  TRY(h->svd_Wl.alloc((size_t)ldl * h->ldk, true));
  TRY(h->svd_lam.alloc((size_t)ldl + h->ldk, true));
  TRY(h->svd_flag.alloc(4, true));
  h->svd_ldl = ldl;
  return 0;
}

// Y[rows of the side, l] = side . Q, with the side's own values or (ganmf_nmf_*) another value array over the same pattern
static int svd_spmm(ganmf_handle* h, const AlsSide& s, const float* Q, float* Y, int l, int ldl, const float* val = nullptr,
                    int tag = T_SVD_SPMM) {
  SvdSpmmP p{};
  p.indptr = s.indptr; p.indices = s.indices; p.val = val ? val : s.conf; p.Q = Q; p.Y = Y; p.ldq = ldl; p.ldy = ldl; p.n_rows = (int)s.rows;
  p.nc4 = (l + 3) / 4;
  const int groups = SVD_SPMM_THREADS / p.nc4;
  p.gpr = groups >= 8 ? 4 : groups;
  p.rows_per_wg = groups >= 8 ? groups / 4 : 1;
  if (s.rows == 0) return 0;
  Scope sc(h, tag, 2.0 * s.nnz * l, 4.0 * s.nnz * l + 8.0 * s.nnz + 4.0 * s.rows * l);
  GANMF_LAUNCH(svd_spmm_kernel, dim3((unsigned)((s.rows + p.rows_per_wg - 1) / p.rows_per_wg)), dim3(SVD_SPMM_THREADS), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the fp32 MFMA whatever the handle's training arithmetic is, as ganmf_als_half_sweep forms its Gram matrix
static int svd_gram(ganmf_handle* h, const float* Y, int rows, int l, int ldl) {
  GemmP g{};
  g.A = Y; g.lda = ldl; g.B = Y; g.ldb = ldl; g.C = h->svd_G; g.ldc = ldl;
  g.M = l; g.N = l; g.K = rows; g.epi.kind = EPI_STORE;
  GemmTune ft;
  ft.mode = MFMA_F32;
  return run_gemm(h, T_SVD_GRAM, T_SVD_GRAM_RED, g, true, true, nullptr, 0, 0, &ft);
}

// C[rows, n] = A[rows, l] . B[l, n]
static int svd_apply(ganmf_handle* h, const float* A, int rows, int l, int ldl, const float* B, int ldb, int n, float* C, int ldc) {
  GemmP g{};
  g.A = A; g.lda = ldl; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
  g.M = rows; g.N = n; g.K = l; g.epi.kind = EPI_STORE;
  GemmTune ft;
  ft.mode = MFMA_F32;
  return run_gemm(h, T_SVD_APPLY, T_SVD_APPLY_RED, g, false, true, nullptr, 0, 0, &ft);
}

// dst = orth(src) by Cholesky-QR applied twice; `other` is the second panel buffer: src -> other -> src
static int svd_cholqr2(ganmf_handle* h, float* src, float* other, int rows, int l, int ldl, int half_step) {
  const size_t shmem = svd_chol_lds_bytes(l);
  TRY(allow_lds((const void*)svd_chol_inv_kernel, shmem));
  float* from = src;
  float* to = other;
  for (int pass = 0; pass < 2; ++pass) {
    TRY(svd_gram(h, from, rows, l, ldl));
    {
      SvdCholP p{};
      p.G = h->svd_G; p.X = h->svd_X; p.ldg = ldl; p.ldx = ldl; p.l = l; p.flag = h->svd_flag; p.code = 1 + 2 * half_step + pass;
      Scope sc(h, T_SVD_CHOL, (double)l * l * l * 2.0 / 3.0, 8.0 * l * l);
      GANMF_LAUNCH(svd_chol_inv_kernel, dim3(1), dim3(SVD_WG), shmem, h->st, p);
      HIP_TRY(hipGetLastError());
    }
    // Q = Y L^-T: B[t][c] = (L^-1)[c][t], the NT form of the product on the dense lower-triangular L^-1
    GemmP g{};
    g.A = from; g.lda = ldl; g.B = h->svd_X; g.ldb = ldl; g.C = to; g.ldc = ldl;
    g.M = rows; g.N = l; g.K = l; g.epi.kind = EPI_STORE;
    GemmTune ft;
    ft.mode = MFMA_F32;
    TRY(run_gemm(h, T_SVD_APPLY, T_SVD_APPLY_RED, g, false, false, nullptr, 0, 0, &ft));
    std::swap(from, to);
  }
  return 0;
}

int ganmf_pure_svd(ganmf_handle* h, const float* omega, int n_random, int n_iter, float* sigma) {
  const char* who = "ganmf_pure_svd";
  if (!h || !omega) return fail(-1, "%s: null argument", who);
  TRY(needs_tensors(h, who));
  TRY(not_cfgan(h, who));
  const int k = h->k, l = n_random, mn = std::min(h->U, h->N);
  if (l < k) return fail(-1, "%s: n_random %d is below num_factors %d", who, l, k);
  if (l > mn) return fail(-1, "%s: n_random %d is above min(num_users, num_items) = %d", who, l, mn);
  if (l > SVD_MAX_RANDOM)
    return fail(-1, "%s: n_random %d is above the limit of %d (the packed triangle of the Cholesky factor has to fit the LDS of a CU)", who, l, SVD_MAX_RANDOM);
  if (n_iter < 0) return fail(-1, "%s: n_iter %d is negative", who, n_iter);
  if (h->has_comm && h->cfg.world_size > 1) return fail(-1, "%s: single-GPU entry", who);
  if (!h->als[0].indptr || !h->als[1].indptr)
    return fail(-1, "%s: ganmf_als_set_confidence has not been called for both sides (the matrix and its transpose)", who);
  for (size_t i = 0; i < (size_t)mn * l; ++i)
    if (!std::isfinite(omega[i])) return fail(-1, "%s: omega[%lld] is not finite", who, (long long)i);
  HIP_TRY(hipSetDevice(h->dev));
  const int ldl = round_up(l, LD_ALIGN);
  TRY(svd_ensure(h, ldl));
  const int ld = h->svd_ldl;      // (the buffers keep the widest leading dimension a call has asked for)
  const bool transposed = h->U < h->N;      // M = URM^T: its rows are the items
  const AlsSide& sM = h->als[transposed ? 1 : 0];
  const AlsSide& sMt = h->als[transposed ? 0 : 1];
  const int m_rows = (int)sM.rows, n_cols = (int)sMt.rows;
  const size_t rows_max = (size_t)std::max(h->U, h->N);
  // pad columns are read as K padding by the products: nothing of an earlier call (another n_random) may be left in them
  HIP_TRY(hipMemsetAsync(h->svd_P[0], 0, rows_max * ld * sizeof(float), h->st));
  HIP_TRY(hipMemsetAsync(h->svd_P[1], 0, rows_max * ld * sizeof(float), h->st));
  HIP_TRY(hipMemsetAsync(h->svd_G, 0, (size_t)ld * ld * sizeof(float), h->st));
  HIP_TRY(hipMemsetAsync(h->svd_X, 0, (size_t)ld * ld * sizeof(float), h->st));
  HIP_TRY(hipMemsetAsync(h->svd_Wl, 0, (size_t)ld * h->ldk * sizeof(float), h->st));
  HIP_TRY(hipMemsetAsync(h->svd_flag, 0, 4 * sizeof(int), h->st));
  HIP_TRY(hipMemcpy2DAsync(h->svd_P[0], (size_t)ld * sizeof(float), omega, (size_t)l * sizeof(float), (size_t)l * sizeof(float), (size_t)mn,
                           hipMemcpyHostToDevice, h->st));
  int cur = 0;      // the panel that holds Q
  auto half = [&](const AlsSide& s, int half_step) -> int {      // Q <- orth(side . Q)
    float* q = h->svd_P[cur];
    float* y = h->svd_P[1 - cur];
    TRY(svd_spmm(h, s, q, y, l, ld));
    TRY(svd_cholqr2(h, y, q, (int)s.rows, l, ld, half_step));      // y -> q -> y
    cur = 1 - cur;
    return 0;
  };
  for (int it = 0; it < n_iter; ++it) {
    TRY(half(sM, 2 * it));
    TRY(half(sMt, 2 * it + 1));
  }
  TRY(half(sM, 2 * n_iter));
  float* const Q = h->svd_P[cur];           // [m_rows, l], orthonormal columns
  float* const Z = h->svd_P[1 - cur];       // [n_cols, l] = M^T Q
  TRY(svd_spmm(h, sMt, Q, Z, l, ld));
  TRY(svd_gram(h, Z, n_cols, l, ld));
  float* const lam = h->svd_lam;
  float* const sig = h->svd_lam + ld;
  {
    SvdEigP p{};
    p.A = h->svd_G; p.lda = ld; p.l = l; p.tol = sqrtf((float)l) * 1.1920929e-7f; p.lam = lam; p.flag = h->svd_flag; p.code = SVD_CODE_EIG;
    Scope sc(h, T_SVD_EIG, 0, 0);
    GANMF_LAUNCH(svd_jacobi_kernel, dim3(1), dim3(SVD_WG), 0, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  {
    SvdSelP p{};
    p.A = h->svd_G; p.lam = lam; p.lda = ld; p.l = l; p.k = k; p.W = h->svd_Wl; p.ldw = h->ldk; p.flag = h->svd_flag; p.code = SVD_CODE_SELECT;
    Scope sc(h, T_SVD_GLUE, 0, 0);
    GANMF_LAUNCH(svd_select_kernel, dim3(1), dim3(SVD_WG), 0, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  int flag[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(flag, h->svd_flag, sizeof flag, hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  const char* advice = "use fewer factors: the matrix has a rank below num_factors + 10, or its leading singular values are too far apart for "
                       "Cholesky-QR in fp32";
  if (flag[0] == SVD_CODE_EIG)
    return fail(-4, "%s: the Jacobi eigensolver of the %d x %d Gram matrix did not converge in %d sweeps; %s", who, l, l, flag[1], advice);
  if (flag[0] == SVD_CODE_SELECT)
    return fail(-4, "%s: final stage: eigenvalue %d of the %d kept is not positive; %s", who, flag[1], k, advice);
  if (flag[0] != 0) {
    const int hs = (flag[0] - 1) / 2, pass = (flag[0] - 1) % 2;
    return fail(-4, "%s: Cholesky-QR broke down in half step %d of %d (%s), pass %d, pivot %d of %d; %s", who, hs, 2 * n_iter + 1,
                hs == 2 * n_iter ? "the final range of M Q" : (hs % 2 == 0 ? "power iteration, M Q" : "power iteration, M^T Q"), pass + 1, flag[1],
                l, advice);
  }
  // nothing can fail in the arithmetic from here on: the factor tensors are written now
  Tensor& Tl = transposed ? h->V : h->Ue;      // left factor: the rows of M
  Tensor& Tr = transposed ? h->Ue : h->V;
  ++h->param_version;
  TRY(svd_apply(h, Q, m_rows, l, ld, h->svd_Wl, h->ldk, k, Tl.p, h->ldk));
  TRY(svd_apply(h, Z, n_cols, l, ld, h->svd_Wl, h->ldk, k, Tr.p, h->ldk));
  {
    SvdFinishP p{};
    p.Uf = h->Ue.p; p.Vf = h->V.p; p.ldu = h->ldk; p.ldv = h->ldk; p.n_users = h->U; p.n_items = h->N; p.transposed = transposed ? 1 : 0;
    p.sigma = sig;
    Scope sc(h, T_SVD_GLUE, 0, 0);
    GANMF_LAUNCH(svd_finish_kernel, dim3((unsigned)k), dim3(256), 0, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  if (sigma) HIP_TRY(hipMemcpyAsync(sigma, sig, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}
