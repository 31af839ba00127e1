// abi_slim.inc -- C ABI: SLIM-BPR trained on a GANMF_MODEL_ITEMSIM handle: ganmf_slim_bpr_init / _draw / _run / _epochs / _finish /
// _get_state (slim_bpr.hpp; the list path: sgd_train.inc).  _finish leaves W held like ganmf_itemknn_fit's and ganmf_p3_fit's.
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static void slim_drop(ganmf_handle* h) {
  SlimState& s = h->slim;
  s = SlimState();
}

static int slim_ready(ganmf_handle* h, const char* who) {
  TRY(itemsim_handle(h, who));
  if (!h->slim.ready) return fail(-1, "%s: ganmf_slim_bpr_init has not been called on this handle", who);
  return 0;
}

int ganmf_slim_bpr_init(ganmf_handle* h, int symmetric, int sgd_mode, double learning_rate, double lambda_i, double lambda_j, double gamma,
                        double beta_1, double beta_2, uint64_t seed, const int64_t* indptr, const int32_t* indices) {
  const char* who = "ganmf_slim_bpr_init";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (sgd_mode < 0 || sgd_mode >= SGD_MODES) return fail(-1, "%s: unknown sgd mode %d", who, sgd_mode);
  if (!std::isfinite(learning_rate) || !std::isfinite(lambda_i) || !std::isfinite(lambda_j))
    return fail(-1, "%s: learning_rate, lambda_i and lambda_j must be finite", who);
  if (sgd_mode == SGD_RMSPROP && !std::isfinite(gamma)) return fail(-1, "%s: gamma must be finite", who);
  if (sgd_mode == SGD_ADAM && !(beta_1 >= 0.0 && beta_1 < 1.0 && beta_2 >= 0.0 && beta_2 < 1.0))
    return fail(-1, "%s: beta_1 and beta_2 must be in [0, 1)", who);
  const int U = h->U, n = h->N;
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (indptr) {
    if (indptr[0] != 0 || indptr[U] < 0 || (indptr[U] > 0 && !indices)) return fail(-1, "%s: bad indptr", who);
    TRY(check_csr(who, indptr, indices, U, n, false, true));
  } else {
    TRY(itemsim_side(h, who, 0));
  }
  SampleProfiles profiles;      // a refusal leaves the state held as it is
  TRY(profiles_upload(profiles, who, U, n, indptr, indices, nullptr, h->als[0].indptr, h->als[0].indices));

  slim_drop(h);
  SlimState& s = h->slim;
  s.profiles = std::move(profiles);
  s.cells = symmetric ? (size_t)n * ((size_t)n + 1) / 2 : (size_t)n * (size_t)n;
  int rc = s.S.alloc(who, symmetric ? "S (one float64 per unordered item pair)" : "S (float64, items x items)", s.cells);
  if (!rc) rc = s.st0.alloc(who, "the optimiser state", (size_t)n);
  if (!rc) rc = s.st1.alloc(who, "the optimiser state", (size_t)n);
  if (rc) { slim_drop(h); return rc; }
  hipError_t e = hipMemset(s.S, 0, s.cells * sizeof(double));
  if (e == hipSuccess) e = hipMemset(s.st0, 0, (size_t)n * sizeof(double));
  if (e == hipSuccess) e = hipMemset(s.st1, 0, (size_t)n * sizeof(double));
  if (e != hipSuccess) { slim_drop(h); return fail(-2, "%s: %s", who, hipGetErrorString(e)); }
  s.symmetric = symmetric ? 1 : 0; s.sgd = sgd_mode;
  s.lr = learning_rate; s.li = lambda_i; s.lj = lambda_j; s.gamma = gamma; s.b1 = beta_1; s.b2 = beta_2;
  s.b1_pow = beta_1; s.b2_pow = beta_2;      // (SLIM_BPR_Cython_Epoch.pyx:161-162)
  s.seed = seed; s.epoch = 0;
  s.ready = true;
  return 0;
}

constexpr int64_t SLIM_WALK_CHUNK = 1 << 16;      // samples per launch of the sequential route

// the list is on the device (t) and, for the levelled route, its items on the host (pos / neg, checked by the caller)
static int slim_run_device(ganmf_handle* h, const char* who, SampleList& t, const int32_t* pos, const int32_t* neg, int64_t n, int mode,
                           int64_t* n_levels) {
  SlimState& s = h->slim;
  if (mode == GANMF_SLIM_AUTO) mode = s.symmetric ? GANMF_SLIM_SEQUENTIAL : GANMF_SLIM_LEVELLED;
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  SlimP p{};
  p.indptr = s.profiles.indptr; p.items = s.profiles.indices; p.S = s.S; p.st0 = s.st0; p.st1 = s.st1;
  p.n_items = h->N; p.symmetric = s.symmetric; p.sgd = s.sgd;
  p.lr = s.lr; p.li = s.li; p.lj = s.lj; p.gamma = s.gamma; p.b1 = s.b1; p.b2 = s.b2;
  p.users = t.users; p.pos = t.pos; p.neg = t.neg;
  double b1p = s.b1_pow, b2p = s.b2_pow;
  if (s.sgd == SGD_ADAM) {      // the powers every sample divides by: one multiplication per sample, as the reference's (:346-347)
    std::vector<double> pows((size_t)2 * n);
    for (int64_t q = 0; q < n; ++q) {
      pows[(size_t)2 * q] = b1p;
      pows[(size_t)2 * q + 1] = b2p;
      b1p *= s.b1;
      b2p *= s.b2;
    }
    TRY(t.pows.alloc(who, "the beta powers", pows.size()));
    HIP_TRY(hipMemcpyAsync(t.pows, pows.data(), pows.size() * sizeof(double), hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));      // (pows leaves scope)
    p.pows = t.pows;
  }
  if (mode == GANMF_SLIM_SEQUENTIAL) {
    for (int64_t first = 0; first < n; first += SLIM_WALK_CHUNK) {
      GANMF_LAUNCH(slim_update_kernel, dim3(1), dim3(SLIM_THREADS), 0, h->st, p, (long long)first,
                   (long long)std::min<int64_t>(SLIM_WALK_CHUNK, n - first), 1);
      HIP_TRY(hipGetLastError());
    }
  } else {
    LevelSchedule sched;
    const int64_t levels = LevelScheduler(h->N).schedule({{pos, 0, h->N}, {neg, 0, h->N}}, n, sched);
    if (levels < 0) return fail(-2, "%s: the schedule met an item id out of range", who);
    TRY(t.upload_order(who, h->st, sched.order));
    p.order = t.order;
    for (int64_t l = 0; l < levels; ++l) {
      const int64_t first = sched.level_start[(size_t)l], count = sched.level_start[(size_t)l + 1] - first;
      GANMF_LAUNCH(slim_update_kernel, dim3((unsigned)count), dim3(SLIM_THREADS), 0, h->st, p, (long long)first, (long long)count, 0);
      HIP_TRY(hipGetLastError());
    }
    if (n_levels) *n_levels = levels;
    HIP_TRY(hipStreamSynchronize(h->st));      // (sched.order leaves scope)
  }
  HIP_TRY(hipStreamSynchronize(h->st));
  s.b1_pow = b1p;
  s.b2_pow = b2p;
  return 0;
}

static int slim_mode_ok(ganmf_handle* h, const char* who, int mode) {
  TRY(sgd_route_ok(who, mode));
  if (mode == GANMF_SLIM_LEVELLED && h->slim.symmetric)
    return fail(-1, "%s: the levelled route needs symmetric = 0 (with one cell per pair a sample's cells lie in the rows of other samples)", who);
  return 0;
}

int ganmf_slim_bpr_draw(ganmf_handle* h, int64_t epoch, int64_t n_epochs, int32_t* users, int32_t* pos, int32_t* neg) {
  const char* who = "ganmf_slim_bpr_draw";
  if (!h || !users || !pos || !neg) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  if (epoch < 0 || n_epochs < 0) return fail(-1, "%s: epoch and n_epochs must be >= 0", who);
  const int64_t per = (int64_t)h->U + 1;
  int64_t n = 0;
  TRY(sample_count(who, n_epochs, per, &n));
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SampleList t;
  TRY(t.alloc(who, n, false));
  TRY(sample_draw(h, h->slim.profiles, false, 0.0, h->slim.seed, epoch, per, n, t));
  return t.download(h->st, n, users, pos, neg, nullptr);
}

int ganmf_slim_bpr_run(ganmf_handle* h, const int32_t* users, const int32_t* pos, const int32_t* neg, int64_t n, int mode, int64_t* n_levels) {
  const char* who = "ganmf_slim_bpr_run";
  if (!h || (n > 0 && (!users || !pos || !neg))) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  TRY(slim_mode_ok(h, who, mode));
  TRY(sample_n_ok(who, n));
  TRY(sample_list_ok(h, who, users, pos, neg, nullptr, n));
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SampleList t;
  TRY(t.upload(who, h->st, n, users, pos, neg, nullptr));
  return slim_run_device(h, who, t, pos, neg, n, mode, n_levels);
}

int ganmf_slim_bpr_epochs(ganmf_handle* h, int64_t n_epochs, int mode, int64_t* n_levels) {
  const char* who = "ganmf_slim_bpr_epochs";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  TRY(slim_mode_ok(h, who, mode));
  if (n_epochs < 0) return fail(-1, "%s: n_epochs must be >= 0", who);
  const int64_t per = (int64_t)h->U + 1;
  int64_t n = 0;
  TRY(sample_count(who, n_epochs, per, &n));
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SampleList t;
  TRY(t.alloc(who, n, false));
  TRY(sample_draw(h, h->slim.profiles, false, 0.0, h->slim.seed, h->slim.epoch, per, n, t));
  std::vector<int32_t> users, pos, neg;
  const bool levelled = mode == GANMF_SLIM_LEVELLED || (mode == GANMF_SLIM_AUTO && !h->slim.symmetric);
  if (levelled) TRY(t.ids_to_host(h->st, n, false, users, pos, neg));
  TRY(slim_run_device(h, who, t, pos.data(), neg.data(), n, mode, n_levels));
  h->slim.epoch += n_epochs;
  return 0;
}

int ganmf_slim_bpr_finish(ganmf_handle* h, int32_t topk, int64_t* nnz_out) {
  const char* who = "ganmf_slim_bpr_finish";
  if (!h || !nnz_out) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  if (topk < 1) return fail(-1, "%s: topk %d must be >= 1", who, topk);
  const int n = h->N, k = std::min<int>(topk, n);
  if (k > GANMF_ITEMKNN_MAX_TOPK)
    return fail(-1, "%s: min(topk, num_items) = %d is above %d (GANMF_ITEMKNN_MAX_TOPK)", who, k, GANMF_ITEMKNN_MAX_TOPK);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  itemsim_drop(h);
  const SlimState& s = h->slim;
  SimPicks t;
  SimCsr R;
  DevBuf<double> rows;      // the private float64 rows of slim_rows_kernel
  // slim_rows_kernel keeps its float64 row in global memory whatever n: at most 512 workgroups.  The column pass takes the plan of the
  // other fits as it is: min(n, 8192) workgroups with the column in LDS, above KNN_ROW_LDS the same 512 with a private float row each.
  const SimRowPlan plan = itemsim_row_plan(n);
  const unsigned grid = (unsigned)std::min(n, 512);
  TRY(rows.alloc(who, "the private float64 rows", (size_t)grid * n));
  TRY(t.alloc(n, k, plan.row_floats()));
  // ---- get_S: the diagonal, then the top-k of every float64 row, rounded to float32 ----
  GANMF_LAUNCH(slim_zero_diag_kernel, dim3((unsigned)((n + SLIM_THREADS - 1) / SLIM_THREADS)), dim3(SLIM_THREADS), 0, h->st, s.S.get(), n, s.symmetric);
  HIP_TRY(hipGetLastError());
  {
    SlimRowP p{};
    p.S = s.S; p.n_items = n; p.symmetric = s.symmetric; p.topk = k; p.rows = rows;
    p.out_idx = t.idx; p.out_val = t.val; p.out_cnt = t.cnt;
    GANMF_LAUNCH(slim_rows_kernel, dim3(grid), dim3(SLIM_THREADS), 0, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  TRY(itemsim_compact(h, who, n, t, k, k, R));
  // ---- similarityMatrixTopK: the k largest non-zeros of every column (p3_columns_kernel, bit copies) ----
  TRY(itemsim_columns(h, n, R, k, plan, t));
  TRY(itemsim_compact(h, who, n, t, k, k, h->knn));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->knn_nnz = h->knn.nnz;
  *nnz_out = h->knn.nnz;
  return 0;
}

int ganmf_slim_bpr_get_state(ganmf_handle* h, double* S, double* state0, double* state1, double* beta_powers, int64_t* epoch) {
  const char* who = "ganmf_slim_bpr_get_state";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  const SlimState& s = h->slim;
  const int n = h->N;
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (S && !s.symmetric) HIP_TRY(hipMemcpy(S, s.S, s.cells * sizeof(double), hipMemcpyDeviceToHost));
  if (S && s.symmetric) {
    std::vector<double> tri(s.cells);
    HIP_TRY(hipMemcpy(tri.data(), s.S, s.cells * sizeof(double), hipMemcpyDeviceToHost));
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b) S[(size_t)a * n + b] = tri[slim_cell(1, n, a, b)];
  }
  if (state0) HIP_TRY(hipMemcpy(state0, s.st0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (state1) HIP_TRY(hipMemcpy(state1, s.st1, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (beta_powers) { beta_powers[0] = s.b1_pow; beta_powers[1] = s.b2_pow; }
  if (epoch) *epoch = s.epoch;
  return 0;
}
