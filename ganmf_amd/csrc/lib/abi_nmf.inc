// abi_nmf.inc -- C ABI: sklearn's NMF solvers on the factor tensors: ganmf_nmf_mu / ganmf_nmf_cd / ganmf_nmf_error
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)
// W is GANMF_T_USER_EMB [U, k], H^T is GANMF_T_ITEM_EMB [N, k]; side 0 of the handle's sparse matrix is X, side 1 is X^T.  A "half"
// updates the factor of side s's rows from the factor of its columns.

static int nmf_gate(ganmf_handle* h, const char* who) {
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(needs_tensors(h, who));
  TRY(not_cfgan(h, who));
  if (h->k > NMF_MAX_FACTORS)
    return fail(-1, "%s: num_factors %d is above the limit of %d (a row of a factor is kept in %d registers per lane of one wave)", who, h->k,
                NMF_MAX_FACTORS, NMF_NT);
  if (h->has_comm && h->cfg.world_size > 1) return fail(-1, "%s: single-GPU entry", who);
  if (!h->als[0].indptr || !h->als[1].indptr)
    return fail(-1, "%s: ganmf_als_set_confidence has not been called for both sides (the matrix and its transpose)", who);
  if (h->als[0].nnz != h->als[1].nnz)
    return fail(-1, "%s: side 0 stores %lld entries and side 1 %lld: side 1 is not the transpose of side 0", who, (long long)h->als[0].nnz,
                (long long)h->als[1].nnz);
  return 0;
}

static int nmf_ensure(ganmf_handle* h, size_t n_scal, size_t n_perm) {
  const size_t rows = (size_t)std::max(h->U, h->N), ld = (size_t)h->ldk, nnz = (size_t)h->als[0].nnz;
  if (!h->nmf_num) TRY(h->nmf_num.alloc(rows * ld, true));
  if (!h->nmf_den) TRY(h->nmf_den.alloc(rows * ld, true));
  if (!h->nmf_G) TRY(h->nmf_G.alloc(2 * ld * ld, true));
  if (!h->nmf_vec) TRY(h->nmf_vec.alloc(2 * ld, true));
  if (!h->nmf_rowd) TRY(h->nmf_rowd.alloc(2 * rows, true));
  if (!h->nmf_part) TRY(h->nmf_part.alloc((size_t)NMF_PARTS, true));
  if (nnz > h->nmf_q.cap || !h->nmf_errp) {      // three arrays by nnz: nmf_errp, allocated last, says that all three are there
    HIP_TRY(hipStreamSynchronize(h->st));
    h->nmf_errp.reset();
    TRY(h->nmf_q.alloc(nnz, true));
    TRY(h->nmf_rowidx.alloc(2 * nnz, true));
    TRY(h->nmf_errp.alloc(2 * ((nnz + NMF_SAMP_CHUNK - 1) / NMF_SAMP_CHUNK), true));
  }
  TRY(h->nmf_scal.grow(h->st, n_scal, true));
  TRY(h->nmf_perm.grow(h->st, n_perm, true));
  return 0;
}

struct NmfHalf {
  const AlsSide* s;
  float* F;          // the factor of the side's rows
  float* O;          // the factor of its columns
  int rows, cols;
  float* G;          // this half's Gram matrix O^T O
  float* vec;        // this half's column sums of O
};
static NmfHalf nmf_half(ganmf_handle* h, int side) {
  NmfHalf v;
  v.s = &h->als[side];
  v.F = side == 0 ? h->Ue.p : h->V.p;
  v.O = side == 0 ? h->V.p : h->Ue.p;
  v.rows = side == 0 ? h->U : h->N;
  v.cols = side == 0 ? h->N : h->U;
  v.G = h->nmf_G + (size_t)side * h->ldk * h->ldk;
  v.vec = h->nmf_vec + (size_t)side * h->ldk;
  return v;
}

// Y[rows of the side, k] = side (with the values `val`) . Q
static int nmf_spmm(ganmf_handle* h, const AlsSide& s, const float* val, const float* Q, float* Y) {
  return svd_spmm(h, s, Q, Y, h->k, h->ldk, val, T_NMF_SPMM);
}

// G = Y^T Y on the fp32 MFMA whatever the handle's training arithmetic is, as ganmf_pure_svd forms its Gram matrices
static int nmf_gram(ganmf_handle* h, const float* Y, int rows, float* G) {
  GemmP g{};
  g.A = Y; g.lda = h->ldk; g.B = Y; g.ldb = h->ldk; g.C = G; g.ldc = h->ldk;
  g.M = h->k; g.N = h->k; g.K = rows; g.epi.kind = EPI_STORE;
  GemmTune ft;
  ft.mode = MFMA_F32;
  return run_gemm(h, T_NMF_GRAM, T_NMF_GRAM_RED, g, true, true, nullptr, 0, 0, &ft);
}

static int nmf_colsum(ganmf_handle* h, const float* A, int rows, float* out) {
  Scope sc(h, T_NMF_REDUCE, 0, 4.0 * rows * h->k);
  GANMF_LAUNCH(nmf_colsum_kernel, dim3((unsigned)((h->k + 63) / 64)), dim3(NMF_SUM_THREADS), 0, h->st, A, h->ldk, rows, h->k, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// out[0] (+)= sum_i in[i * stride]
static int nmf_sum(ganmf_handle* h, const double* in, long long n, int stride, double* out, int add) {
  Scope sc(h, T_NMF_REDUCE, 0, 8.0 * n);
  GANMF_LAUNCH(nmf_sum_kernel, dim3(1), dim3(NMF_SUM_THREADS), 0, h->st, in, n, stride, out, add);
  HIP_TRY(hipGetLastError());
  return 0;
}

// out[0] = sum A . B over [rows, cols] (elements with a flat index below `total`)
static int nmf_dot(ganmf_handle* h, const float* A, int lda, const float* B, int ldb, int rows, int cols, long long total, double* out) {
  {
    Scope sc(h, T_NMF_REDUCE, 2.0 * total, 8.0 * total);
    GANMF_LAUNCH(nmf_dot_kernel, dim3(NMF_PARTS), dim3(NMF_THREADS), 0, h->st, A, lda, B, ldb, rows, cols, total, h->nmf_part.get());
    HIP_TRY(hipGetLastError());
  }
  return nmf_sum(h, h->nmf_part, NMF_PARTS, 1, out, 0);
}

// F *= num / den: den = F . G on the fp32 MFMA (G symmetric: the K-major B of the NN product), or the broadcast vector `den`
static int nmf_mu_rows(ganmf_handle* h, const NmfHalf& v, const float* G, const float* den, float zero_den, int floor_h) {
  const int k = h->k;
  if (v.rows == 0) return 0;
  NmfMuP p{};
  p.F = v.F; p.num = h->nmf_num; p.den = den; p.ldf = h->ldk; p.ldn = h->ldk; p.ldd = 0; p.rows = v.rows; p.k = k;
  p.zero_den = zero_den; p.floor_h = floor_h;
  if (G) {
    GemmP g{};
    g.A = v.F; g.lda = h->ldk; g.B = G; g.ldb = h->ldk; g.C = h->nmf_den; g.ldc = h->ldk;
    g.M = v.rows; g.N = k; g.K = k; g.epi.kind = EPI_STORE;
    GemmTune ft;
    ft.mode = MFMA_F32;
    TRY(run_gemm(h, T_NMF_MU_ROWS, T_NMF_MU_ROWS, g, false, true, nullptr, 0, 0, &ft));
    p.den = h->nmf_den; p.ldd = h->ldk;
  }
  const long long blocks = ((long long)v.rows * k + NMF_THREADS - 1) / NMF_THREADS;
  Scope sc(h, T_NMF_MU_ROWS, 2.0 * v.rows * k, 16.0 * v.rows * k);
  GANMF_LAUNCH(nmf_mu_kernel, dim3((unsigned)std::min<long long>(blocks, 4096)), dim3(NMF_THREADS), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the row of every CSR position of both sides, for nmf_sampled_kernel: formed once per call of an entry that runs it
static int nmf_rowidx_build(ganmf_handle* h) {
  for (int side = 0; side < 2; ++side) {
    const AlsSide& s = h->als[side];
    if (s.rows == 0 || s.nnz == 0) continue;
    Scope sc(h, T_NMF_SAMPLED, 0, 4.0 * s.nnz);
    GANMF_LAUNCH(nmf_rowidx_kernel, dim3((unsigned)((s.rows + 3) / 4)), dim3(NMF_THREADS), 0, h->st, s.indptr.get(), (int)s.rows,
                 h->nmf_rowidx + (size_t)side * s.nnz);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// q (and, with err, the chunks' divergence sums) of one side from the factors as they stand
static int nmf_sampled(ganmf_handle* h, int side, float* q, double* err) {
  const NmfHalf v = nmf_half(h, side);
  const long long nnz = v.s->nnz;
  NmfSampP p{};
  p.rowidx = h->nmf_rowidx + (size_t)side * nnz; p.indices = v.s->indices; p.x = v.s->conf; p.A = v.F; p.Bm = v.O; p.q = q; p.err = err;
  p.nnz = nnz; p.lda = h->ldk; p.ldb = h->ldk; p.nc4 = (h->k + 3) / 4;
  p.lanes = p.nc4 <= 4 ? 4 : (p.nc4 <= 8 ? 8 : 16);
  if (nnz == 0) return 0;
  const long long chunks = (nnz + NMF_SAMP_CHUNK - 1) / NMF_SAMP_CHUNK;
  Scope sc(h, T_NMF_SAMPLED, 2.0 * nnz * h->k, 8.0 * nnz * h->k + 16.0 * nnz);
  GANMF_LAUNCH(nmf_sampled_kernel, dim3((unsigned)((chunks + 3) / 4)), dim3(NMF_THREADS), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The error of the factors as they stand, enqueued; *error is final after nmf_error_finish behind a synchronise.
//   Frobenius: scal[0] = |X|^2, scal[1] = tr((W^T W)(H H^T)), scal[2] = tr((X H^T) W^T)
//   Kullback-Leibler: scal[0] = sum x log(x / max(wh, EPS)), scal[1] = sum x (both over x > EPS); vec = colsum(H^T) | colsum(W)
static int nmf_error_enqueue(ganmf_handle* h, int beta_loss) {
  const NmfHalf w = nmf_half(h, 0), t = nmf_half(h, 1);
  double* scal = h->nmf_scal;
  if (beta_loss == GANMF_NMF_FROBENIUS) {
    const long long nnz = w.s->nnz;
    TRY(nmf_dot(h, w.s->conf, 4096, w.s->conf, 4096, (int)((nnz + 4095) / 4096), 4096, nnz, scal + 0));
    TRY(nmf_gram(h, w.O, w.cols, w.G));      // H H^T
    TRY(nmf_gram(h, t.O, t.cols, t.G));      // W^T W
    TRY(nmf_dot(h, w.G, h->ldk, t.G, h->ldk, h->k, h->k, (long long)h->k * h->k, scal + 1));
    TRY(nmf_spmm(h, *w.s, w.s->conf, w.O, h->nmf_num));
    TRY(nmf_dot(h, h->nmf_num, h->ldk, w.F, h->ldk, w.rows, h->k, (long long)w.rows * h->k, scal + 2));
  } else {
    const long long chunks = (w.s->nnz + NMF_SAMP_CHUNK - 1) / NMF_SAMP_CHUNK;
    TRY(nmf_sampled(h, 0, nullptr, h->nmf_errp));
    TRY(nmf_sum(h, h->nmf_errp, chunks, 2, scal + 0, 0));
    TRY(nmf_sum(h, h->nmf_errp + 1, chunks, 2, scal + 1, 0));
    TRY(nmf_colsum(h, w.O, w.cols, w.vec));
    TRY(nmf_colsum(h, t.O, t.cols, t.vec));
  }
  return 0;
}

static int nmf_error_finish(ganmf_handle* h, int beta_loss, double* error) {
  double scal[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(scal, h->nmf_scal, sizeof scal, hipMemcpyDeviceToHost, h->st));
  std::vector<float> vec(2 * (size_t)h->ldk, 0.f);
  if (beta_loss != GANMF_NMF_FROBENIUS)
    HIP_TRY(hipMemcpyAsync(vec.data(), h->nmf_vec, vec.size() * sizeof(float), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  double r;
  if (beta_loss == GANMF_NMF_FROBENIUS) {
    r = scal[0] + scal[1] - 2.0 * scal[2];
  } else {
    double sum_wh = 0.0;
    for (int c = 0; c < h->k; ++c) sum_wh += (double)vec[c] * (double)vec[h->ldk + c];
    r = 2.0 * (scal[0] + sum_wh - scal[1]);
  }
  *error = std::sqrt(std::max(r, 0.0));
  return 0;
}

static int nmf_beta_ok(const char* who, int beta_loss) {
  if (beta_loss != GANMF_NMF_FROBENIUS && beta_loss != GANMF_NMF_KULLBACK_LEIBLER)
    return fail(-1, "%s: beta_loss must be GANMF_NMF_FROBENIUS (0) or GANMF_NMF_KULLBACK_LEIBLER (1), given %d", who, beta_loss);
  return 0;
}

int ganmf_nmf_error(ganmf_handle* h, int beta_loss, double* error) {
  const char* who = "ganmf_nmf_error";
  TRY(nmf_gate(h, who));
  if (!error) return fail(-1, "%s: null argument", who);
  TRY(nmf_beta_ok(who, beta_loss));
  HIP_TRY(hipSetDevice(h->dev));
  TRY(nmf_ensure(h, 4, 0));
  if (beta_loss == GANMF_NMF_KULLBACK_LEIBLER) TRY(nmf_rowidx_build(h));
  TRY(nmf_error_enqueue(h, beta_loss));
  return nmf_error_finish(h, beta_loss, error);
}

int ganmf_nmf_mu(ganmf_handle* h, int beta_loss, int n_iter, int update_H, double* error) {
  const char* who = "ganmf_nmf_mu";
  TRY(nmf_gate(h, who));
  TRY(nmf_beta_ok(who, beta_loss));
  if (n_iter < 0) return fail(-1, "%s: n_iter %d is negative", who, n_iter);
  HIP_TRY(hipSetDevice(h->dev));
  TRY(nmf_ensure(h, 4, 0));
  const NmfHalf w = nmf_half(h, 0), t = nmf_half(h, 1);
  const bool kl = beta_loss == GANMF_NMF_KULLBACK_LEIBLER;
  if (kl) TRY(nmf_rowidx_build(h));
  if (n_iter > 0) ++h->param_version;
  for (int it = 0; it < n_iter; ++it) {
    const bool fresh = update_H || it == 0;      // with H fixed, X H^T, H H^T and the column sums of H^T are formed once
    if (kl) {
      if (fresh) TRY(nmf_colsum(h, w.O, w.cols, w.vec));
      TRY(nmf_sampled(h, 0, h->nmf_q, nullptr));
      TRY(nmf_spmm(h, *w.s, h->nmf_q, w.O, h->nmf_num));
      TRY(nmf_mu_rows(h, w, nullptr, w.vec, NMF_EPS, 0));
    } else {
      if (fresh) {
        TRY(nmf_gram(h, w.O, w.cols, w.G));
        TRY(nmf_spmm(h, *w.s, w.s->conf, w.O, h->nmf_num));
      }
      TRY(nmf_mu_rows(h, w, w.G, nullptr, NMF_EPS, 0));
    }
    if (!update_H) continue;
    if (kl) {
      TRY(nmf_sampled(h, 1, h->nmf_q, nullptr));      // Q again, from the new W
      TRY(nmf_spmm(h, *t.s, h->nmf_q, t.O, h->nmf_num));
      TRY(nmf_colsum(h, t.O, t.cols, t.vec));
      TRY(nmf_mu_rows(h, t, nullptr, t.vec, 1.0f, 1));
    } else {
      TRY(nmf_gram(h, t.O, t.cols, t.G));
      TRY(nmf_spmm(h, *t.s, t.s->conf, t.O, h->nmf_num));
      TRY(nmf_mu_rows(h, t, t.G, nullptr, NMF_EPS, 0));
    }
  }
  if (error) {
    TRY(nmf_error_enqueue(h, beta_loss));
    return nmf_error_finish(h, beta_loss, error);
  }
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}

// one half of a coordinate-descent iteration: out[0] (+)= the half's violation
static int nmf_cd_half(ganmf_handle* h, const NmfHalf& v, const int* perm, bool fresh, double* out, int add) {
  const int k = h->k;
  if (fresh) {
    TRY(nmf_gram(h, v.O, v.cols, v.G));
    TRY(nmf_spmm(h, *v.s, v.s->conf, v.O, h->nmf_num));
  }
  NmfCdP p{};
  p.F = v.F; p.B = h->nmf_num; p.G = v.G; p.perm = perm; p.viol = h->nmf_rowd; p.ldf = h->ldk; p.ldb = h->ldk; p.ldg = h->ldk;
  p.rows = v.rows; p.k = k;
  if (v.rows > 0) {
    Scope sc(h, T_NMF_CD_ROWS, 2.0 * v.rows * k * k, 4.0 * v.rows * k * (k + 3.0));
    const dim3 grid((unsigned)((v.rows + 3) / 4)), block(NMF_THREADS);
    switch ((k + 63) / 64) {
      case 1: GANMF_LAUNCH(nmf_cd_rows_kernel<1>, grid, block, 0, h->st, p); break;
      case 2: GANMF_LAUNCH(nmf_cd_rows_kernel<2>, grid, block, 0, h->st, p); break;
      case 3: GANMF_LAUNCH(nmf_cd_rows_kernel<3>, grid, block, 0, h->st, p); break;
      case 4: GANMF_LAUNCH(nmf_cd_rows_kernel<4>, grid, block, 0, h->st, p); break;
      default: GANMF_LAUNCH(nmf_cd_rows_kernel<NMF_NT>, grid, block, 0, h->st, p);
    }
    HIP_TRY(hipGetLastError());
  }
  return nmf_sum(h, h->nmf_rowd, v.rows, 1, out, add);
}

int ganmf_nmf_cd(ganmf_handle* h, const int32_t* perms, int n_iter, int update_H, double* violation) {
  const char* who = "ganmf_nmf_cd";
  TRY(nmf_gate(h, who));
  if (n_iter < 0) return fail(-1, "%s: n_iter %d is negative", who, n_iter);
  if (n_iter > 0 && (!perms || !violation)) return fail(-1, "%s: null argument", who);
  const int k = h->k, halves = update_H ? 2 : 1;
  const size_t n_perm = (size_t)n_iter * halves * k;
  std::vector<char> seen((size_t)k);
  for (size_t b = 0; b < (size_t)n_iter * halves; ++b) {
    std::fill(seen.begin(), seen.end(), 0);
    for (int i = 0; i < k; ++i) {
      const int32_t t = perms[b * k + i];
      if (t < 0 || t >= k || seen[t])
        return fail(-1, "%s: permutation %lld is not a permutation of 0 .. %d (entry %d is %d)", who, (long long)b, k - 1, i, (int)t);
      seen[t] = 1;
    }
  }
  HIP_TRY(hipSetDevice(h->dev));
  TRY(nmf_ensure(h, 4 + (size_t)n_iter, n_perm));
  if (n_iter == 0) return 0;
  const NmfHalf w = nmf_half(h, 0), t = nmf_half(h, 1);
  HIP_TRY(hipMemcpyAsync(h->nmf_perm, perms, n_perm * sizeof(int), hipMemcpyHostToDevice, h->st));
  ++h->param_version;
  double* viol = h->nmf_scal + 4;
  for (int it = 0; it < n_iter; ++it) {
    const int* pm = h->nmf_perm + (size_t)it * halves * k;
    TRY(nmf_cd_half(h, w, pm, update_H || it == 0, viol + it, 0));
    if (update_H) TRY(nmf_cd_half(h, t, pm + k, true, viol + it, 1));
  }
  HIP_TRY(hipMemcpyAsync(violation, viol, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}
