// abi_slim.inc -- C ABI: SLIM-BPR trained on a GANMF_MODEL_ITEMSIM handle: ganmf_slim_bpr_init / _draw / _run / _epochs / _finish /
// _get_state (slim_bpr.hpp, slim_sched.hpp).  _finish leaves W held like ganmf_itemknn_fit's and ganmf_p3_fit's.
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static_assert(SLIM_SGD == GANMF_SLIM_SGD && SLIM_ADAGRAD == GANMF_SLIM_ADAGRAD && SLIM_RMSPROP == GANMF_SLIM_RMSPROP &&
              SLIM_ADAM == GANMF_SLIM_ADAM, "sgd modes of the kernels and of the header");

static void slim_drop(ganmf_handle* h) {
  SlimState& s = h->slim;
  hipFree(s.S); hipFree(s.st0); hipFree(s.st1); hipFree(s.indptr); hipFree(s.items); hipFree(s.eligible);
  s = SlimState();
}

static int slim_ready(ganmf_handle* h, const char* who) {
  TRY(itemsim_handle(h, who));
  if (!h->slim.ready) return fail(-1, "%s: ganmf_slim_bpr_init has not been called on this handle", who);
  return 0;
}

// hipMalloc whose failure names the bytes asked for (and is cleared: the handle stays usable)
static int slim_alloc(const char* who, const char* what, void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 8));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return fail(-2, "%s: out of memory: %s needs %llu bytes (%s)", who, what, (unsigned long long)bytes, hipGetErrorString(e));
  }
  return 0;
}

int ganmf_slim_bpr_init(ganmf_handle* h, int symmetric, int sgd_mode, double learning_rate, double lambda_i, double lambda_j, double gamma,
                        double beta_1, double beta_2, uint64_t seed, const int64_t* indptr, const int32_t* indices) {
  const char* who = "ganmf_slim_bpr_init";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (sgd_mode < 0 || sgd_mode >= SLIM_SGD_MODES) return fail(-1, "%s: unknown sgd mode %d", who, sgd_mode);
  if (!std::isfinite(learning_rate) || !std::isfinite(lambda_i) || !std::isfinite(lambda_j))
    return fail(-1, "%s: learning_rate, lambda_i and lambda_j must be finite", who);
  if (sgd_mode == SLIM_RMSPROP && !std::isfinite(gamma)) return fail(-1, "%s: gamma must be finite", who);
  if (sgd_mode == SLIM_ADAM && !(beta_1 >= 0.0 && beta_1 < 1.0 && beta_2 >= 0.0 && beta_2 < 1.0))
    return fail(-1, "%s: beta_1 and beta_2 must be in [0, 1)", who);
  const int U = h->U, n = h->N;
  std::vector<int64_t> ip((size_t)U + 1);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (indptr) {
    if (indptr[0] != 0 || indptr[U] < 0 || (indptr[U] > 0 && !indices)) return fail(-1, "%s: bad indptr", who);
    TRY(check_csr(who, indptr, indices, U, n, false, true));
    std::copy(indptr, indptr + U + 1, ip.begin());
  } else {
    TRY(itemsim_side(h, who, 0));
    static_assert(sizeof(long long) == sizeof(int64_t), "indptr words");
    HIP_TRY(hipMemcpy(ip.data(), h->als[0].indptr, ip.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  std::vector<int> eligible;
  for (int u = 0; u < U; ++u) {
    const int64_t len = ip[(size_t)u + 1] - ip[(size_t)u];
    if (len > 0 && len < n) eligible.push_back(u);
  }
  if (eligible.empty()) return fail(-1, "%s: no user has a profile that is neither empty nor full: there is nothing to sample", who);

  slim_drop(h);
  SlimState& s = h->slim;
  const size_t nnz = (size_t)ip[(size_t)U];
  s.cells = symmetric ? (size_t)n * ((size_t)n + 1) / 2 : (size_t)n * (size_t)n;
  int rc = slim_alloc(who, symmetric ? "S (one float64 per unordered item pair)" : "S (float64, items x items)", (void**)&s.S, s.cells * sizeof(double));
  if (!rc) rc = slim_alloc(who, "the optimiser state", (void**)&s.st0, (size_t)n * sizeof(double));
  if (!rc) rc = slim_alloc(who, "the optimiser state", (void**)&s.st1, (size_t)n * sizeof(double));
  if (!rc) rc = slim_alloc(who, "the profiles", (void**)&s.indptr, ip.size() * sizeof(long long));
  if (!rc) rc = slim_alloc(who, "the profiles", (void**)&s.items, nnz * sizeof(int));
  if (!rc) rc = slim_alloc(who, "the eligible users", (void**)&s.eligible, eligible.size() * sizeof(int));
  if (rc) { slim_drop(h); return rc; }
  hipError_t e = hipMemset(s.S, 0, s.cells * sizeof(double));
  if (e == hipSuccess) e = hipMemset(s.st0, 0, (size_t)n * sizeof(double));
  if (e == hipSuccess) e = hipMemset(s.st1, 0, (size_t)n * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(s.indptr, ip.data(), ip.size() * sizeof(long long), hipMemcpyHostToDevice);
  if (e == hipSuccess && nnz)
    e = indptr ? hipMemcpy(s.items, indices, nnz * sizeof(int), hipMemcpyHostToDevice)
               : hipMemcpy(s.items, h->als[0].indices, nnz * sizeof(int), hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(s.eligible, eligible.data(), eligible.size() * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) { slim_drop(h); return fail(-2, "%s: %s", who, hipGetErrorString(e)); }
  s.n_eligible = (int)eligible.size();
  s.symmetric = symmetric ? 1 : 0; s.sgd = sgd_mode;
  s.lr = learning_rate; s.li = lambda_i; s.lj = lambda_j; s.gamma = gamma; s.b1 = beta_1; s.b2 = beta_2;
  s.b1_pow = beta_1; s.b2_pow = beta_2;      // (SLIM_BPR_Cython_Epoch.pyx:161-162)
  s.seed = seed; s.epoch = 0;
  s.ready = true;
  return 0;
}

// n = n_epochs * (num_users + 1) triples of the epochs [epoch, epoch + n_epochs) into device arrays
static int slim_draw_device(ganmf_handle* h, int64_t epoch, int64_t n, int* users, int* pos, int* neg) {
  const SlimState& s = h->slim;
  SlimDrawP p{};
  p.indptr = s.indptr; p.items = s.items; p.eligible = s.eligible;
  p.n_users = h->U; p.n_items = h->N; p.n_eligible = s.n_eligible;
  p.seed = s.seed; p.epoch0 = epoch; p.per_epoch = (long long)h->U + 1; p.n = n;
  p.users = users; p.pos = pos; p.neg = neg;
  const unsigned blocks = (unsigned)((n + SLIM_THREADS - 1) / SLIM_THREADS);
  GANMF_LAUNCH(slim_draw_kernel, dim3(blocks), dim3(SLIM_THREADS), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

struct SlimRunTmp {
  int *users = nullptr, *pos = nullptr, *neg = nullptr;
  double* pows = nullptr;
  long long* order = nullptr;
  ~SlimRunTmp() { hipFree(users); hipFree(pos); hipFree(neg); hipFree(pows); hipFree(order); }
};

constexpr int64_t SLIM_MAX_SAMPLES = (int64_t)1 << 30;
constexpr int64_t SLIM_WALK_CHUNK = 1 << 16;      // samples per launch of the sequential route

// the list is on the device (t.users / t.pos / t.neg) and its items on the host (pos / neg, checked by the caller)
static int slim_run_device(ganmf_handle* h, const char* who, SlimRunTmp& t, const int32_t* pos, const int32_t* neg, int64_t n, int mode,
                           int64_t* n_levels) {
  SlimState& s = h->slim;
  if (mode == GANMF_SLIM_AUTO) mode = s.symmetric ? GANMF_SLIM_SEQUENTIAL : GANMF_SLIM_LEVELLED;
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  SlimP p{};
  p.indptr = s.indptr; p.items = s.items; p.S = s.S; p.st0 = s.st0; p.st1 = s.st1;
  p.n_items = h->N; p.symmetric = s.symmetric; p.sgd = s.sgd;
  p.lr = s.lr; p.li = s.li; p.lj = s.lj; p.gamma = s.gamma; p.b1 = s.b1; p.b2 = s.b2;
  p.users = t.users; p.pos = t.pos; p.neg = t.neg;
  double b1p = s.b1_pow, b2p = s.b2_pow;
  if (s.sgd == SLIM_ADAM) {      // the powers every sample divides by: one multiplication per sample, as the reference's (:346-347)
    std::vector<double> pows((size_t)2 * n);
    for (int64_t q = 0; q < n; ++q) {
      pows[(size_t)2 * q] = b1p;
      pows[(size_t)2 * q + 1] = b2p;
      b1p *= s.b1;
      b2p *= s.b2;
    }
    TRY(slim_alloc(who, "the beta powers", (void**)&t.pows, pows.size() * sizeof(double)));
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
    SlimSchedule sched;
    const int64_t levels = slim_schedule(pos, neg, n, h->N, sched);
    if (levels < 0) return fail(-2, "%s: the schedule met an item id out of range", who);
    TRY(slim_alloc(who, "the level order", (void**)&t.order, (size_t)n * sizeof(long long)));
    static_assert(sizeof(long long) == sizeof(int64_t), "order words");
    HIP_TRY(hipMemcpyAsync(t.order, sched.order.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice, h->st));
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
  if (mode != GANMF_SLIM_AUTO && mode != GANMF_SLIM_SEQUENTIAL && mode != GANMF_SLIM_LEVELLED) return fail(-1, "%s: unknown route %d", who, mode);
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
  if (n_epochs > SLIM_MAX_SAMPLES / per) return fail(-1, "%s: more than 2^30 samples in one call", who);
  const int64_t n = n_epochs * per;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SlimRunTmp t;
  TRY(slim_alloc(who, "the samples", (void**)&t.users, (size_t)n * sizeof(int)));
  TRY(slim_alloc(who, "the samples", (void**)&t.pos, (size_t)n * sizeof(int)));
  TRY(slim_alloc(who, "the samples", (void**)&t.neg, (size_t)n * sizeof(int)));
  TRY(slim_draw_device(h, epoch, n, t.users, t.pos, t.neg));
  HIP_TRY(hipMemcpyAsync(users, t.users, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipMemcpyAsync(pos, t.pos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipMemcpyAsync(neg, t.neg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}

int ganmf_slim_bpr_run(ganmf_handle* h, const int32_t* users, const int32_t* pos, const int32_t* neg, int64_t n, int mode, int64_t* n_levels) {
  const char* who = "ganmf_slim_bpr_run";
  if (!h || (n > 0 && (!users || !pos || !neg))) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  TRY(slim_mode_ok(h, who, mode));
  if (n < 0 || n > SLIM_MAX_SAMPLES) return fail(-1, "%s: n out of range", who);
  for (int64_t q = 0; q < n; ++q) {
    if (users[q] < 0 || users[q] >= h->U) return fail(-1, "%s: sample %lld names user %d of %d", who, (long long)q, users[q], h->U);
    if (pos[q] < 0 || pos[q] >= h->N || neg[q] < 0 || neg[q] >= h->N)
      return fail(-1, "%s: sample %lld names item %d / %d of %d", who, (long long)q, pos[q], neg[q], h->N);
    if (pos[q] == neg[q]) return fail(-1, "%s: sample %lld has the same positive and negative item %d", who, (long long)q, pos[q]);
  }
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SlimRunTmp t;
  TRY(slim_alloc(who, "the samples", (void**)&t.users, (size_t)n * sizeof(int)));
  TRY(slim_alloc(who, "the samples", (void**)&t.pos, (size_t)n * sizeof(int)));
  TRY(slim_alloc(who, "the samples", (void**)&t.neg, (size_t)n * sizeof(int)));
  HIP_TRY(hipMemcpyAsync(t.users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->st));
  HIP_TRY(hipMemcpyAsync(t.pos, pos, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->st));
  HIP_TRY(hipMemcpyAsync(t.neg, neg, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->st));
  return slim_run_device(h, who, t, pos, neg, n, mode, n_levels);
}

int ganmf_slim_bpr_epochs(ganmf_handle* h, int64_t n_epochs, int mode, int64_t* n_levels) {
  const char* who = "ganmf_slim_bpr_epochs";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(slim_ready(h, who));
  TRY(slim_mode_ok(h, who, mode));
  if (n_epochs < 0) return fail(-1, "%s: n_epochs must be >= 0", who);
  const int64_t per = (int64_t)h->U + 1;
  if (n_epochs > SLIM_MAX_SAMPLES / per) return fail(-1, "%s: more than 2^30 samples in one call", who);
  const int64_t n = n_epochs * per;
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SlimRunTmp t;
  TRY(slim_alloc(who, "the samples", (void**)&t.users, (size_t)n * sizeof(int)));
  TRY(slim_alloc(who, "the samples", (void**)&t.pos, (size_t)n * sizeof(int)));
  TRY(slim_alloc(who, "the samples", (void**)&t.neg, (size_t)n * sizeof(int)));
  TRY(slim_draw_device(h, h->slim.epoch, n, t.users, t.pos, t.neg));
  std::vector<int32_t> pos, neg;
  const bool levelled = mode == GANMF_SLIM_LEVELLED || (mode == GANMF_SLIM_AUTO && !h->slim.symmetric);
  if (levelled) {      // the one copy back of the call: the items the schedule is formed from
    pos.resize((size_t)n);
    neg.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(pos.data(), t.pos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipMemcpyAsync(neg.data(), t.neg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
  }
  TRY(slim_run_device(h, who, t, pos.data(), neg.data(), n, mode, n_levels));
  h->slim.epoch += n_epochs;
  return 0;
}

struct SlimFinishTmp {
  double* rows = nullptr;
  ~SlimFinishTmp() { hipFree(rows); }
};

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
  SlimFinishTmp d;
  // slim_rows_kernel keeps its float64 row in global memory whatever n: at most 512 workgroups.  The column pass takes the plan of the
  // other fits as it is: min(n, 8192) workgroups with the column in LDS, above KNN_ROW_LDS the same 512 with a private float row each.
  const SimRowPlan plan = itemsim_row_plan(n);
  const unsigned grid = (unsigned)std::min(n, 512);
  TRY(slim_alloc(who, "the private float64 rows", (void**)&d.rows, (size_t)grid * n * sizeof(double)));
  TRY(t.alloc(n, k, plan.row_floats()));
  // ---- get_S: the diagonal, then the top-k of every float64 row, rounded to float32 ----
  GANMF_LAUNCH(slim_zero_diag_kernel, dim3((unsigned)((n + SLIM_THREADS - 1) / SLIM_THREADS)), dim3(SLIM_THREADS), 0, h->st, s.S, n, s.symmetric);
  HIP_TRY(hipGetLastError());
  {
    SlimRowP p{};
    p.S = s.S; p.n_items = n; p.symmetric = s.symmetric; p.topk = k; p.rows = d.rows;
    p.out_idx = t.idx; p.out_val = t.val; p.out_cnt = t.cnt;
    GANMF_LAUNCH(slim_rows_kernel, dim3(grid), dim3(SLIM_THREADS), 0, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  TRY(itemsim_compact(h, who, t, k, k, &R.indptr, &R.idx, &R.val, &R.nnz));
  // ---- similarityMatrixTopK: the k largest non-zeros of every column (p3_columns_kernel, bit copies) ----
  TRY(itemsim_columns(h, R, k, plan, t));
  long long nnz = 0;
  TRY(itemsim_compact(h, who, t, k, k, &h->knn_indptr, &h->knn_nbr, &h->knn_val, &nnz));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->knn_nnz = nnz;
  *nnz_out = nnz;
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
