// abi_mf_sgd.inc -- C ABI: MF-BPR and FunkSVD trained on a GANMF_MODEL_MF handle: ganmf_mf_sgd_init / _draw / _run / _epochs /
// _publish / _get_state / _set_state (mf_sgd.hpp; the list path: sgd_train.inc).  _publish rounds the float64 state into the handle's
// factor tensors.
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static_assert(MF_SGD_BPR == GANMF_MF_SGD_BPR && MF_SGD_FUNK == GANMF_MF_SGD_FUNK, "algorithms of the kernels and of the header");

static void mf_sgd_drop(ganmf_handle* h) {
  MfSgdState& s = h->mfs;
  s = MfSgdState();
}

static int mf_sgd_handle(ganmf_handle* h, const char* who) {
  if (h->cfg.model != GANMF_MODEL_MF) return fail(-1, "%s: needs a GANMF_MODEL_MF handle", who);
  if (h->has_comm && h->cfg.world_size > 1) return fail(-1, "%s: single-GPU entry", who);
  return 0;
}

static int mf_sgd_ready(ganmf_handle* h, const char* who) {
  TRY(mf_sgd_handle(h, who));
  if (!h->mfs.ready) return fail(-1, "%s: ganmf_mf_sgd_init has not been called on this handle", who);
  return 0;
}

// the pointers of block `b` (0 parameters, 1 st0, 2 st1) of the state
static void mf_sgd_block(const ganmf_handle* h, int b, double** W, double** H, double** ub, double** ib, double** gb) {
  const MfSgdState& s = h->mfs;
  double* base = s.P + (size_t)b * s.block;
  *W = base;
  *H = *W + (size_t)h->U * s.k;
  *ub = *H + (size_t)h->N * s.k;
  *ib = *ub + h->U;
  *gb = *ib + h->N;
}

int ganmf_mf_sgd_init(ganmf_handle* h, int algorithm, int use_bias, int sgd_mode, double learning_rate, double user_reg, double item_reg,
                      double positive_reg, double negative_reg, double bias_reg, double negative_interactions_quota, uint64_t seed,
                      const int64_t* indptr, const int32_t* indices, const double* ratings, const double* user_factors,
                      const double* item_factors) {
  const char* who = "ganmf_mf_sgd_init";
  if (!h || !indptr || !user_factors || !item_factors) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_handle(h, who));
  if (algorithm < 0 || algorithm >= MF_SGD_ALGOS) return fail(-1, "%s: unknown algorithm %d", who, algorithm);
  if (sgd_mode < 0 || sgd_mode >= SGD_MODES) return fail(-1, "%s: unknown sgd mode %d", who, sgd_mode);
  use_bias = use_bias ? 1 : 0;
  if (use_bias && algorithm == MF_SGD_BPR) return fail(-1, "%s: MF_BPR has no biases (the reference's class forces use_bias = False)", who);
  const int U = h->U, n = h->N, k = h->k - 2 * use_bias;
  if (k < 1) return fail(-1, "%s: with use_bias the handle needs num_factors + 2 columns; it has %d", who, h->k);
  if (h->k > GANMF_MF_SGD_MAX_FACTORS)
    return fail(-1, "%s: the handle has %d factor columns, above %d (GANMF_MF_SGD_MAX_FACTORS)", who, h->k, GANMF_MF_SGD_MAX_FACTORS);
  if (!std::isfinite(learning_rate) || !std::isfinite(user_reg) || !std::isfinite(item_reg) || !std::isfinite(positive_reg) ||
      !std::isfinite(negative_reg) || !std::isfinite(bias_reg))
    return fail(-1, "%s: learning_rate and the regularisation weights must be finite", who);
  if (!(negative_interactions_quota >= 0.0 && negative_interactions_quota < 1.0))
    return fail(-1, "%s: negative_interactions_quota must be in [0, 1)", who);
  if (indptr[0] != 0 || indptr[U] < 0 || (indptr[U] > 0 && (!indices || !ratings))) return fail(-1, "%s: bad indptr", who);
  TRY(check_csr(who, indptr, indices, U, n, false, true));
  const size_t nnz = (size_t)indptr[U];
  for (size_t q = 0; q < nnz; ++q)
    if (!std::isfinite(ratings[q])) return fail(-1, "%s: rating %llu is not finite", who, (unsigned long long)q);
  for (size_t q = 0; q < (size_t)U * k; ++q)
    if (!std::isfinite(user_factors[q])) return fail(-1, "%s: the initial user factors are not finite", who);
  for (size_t q = 0; q < (size_t)n * k; ++q)
    if (!std::isfinite(item_factors[q])) return fail(-1, "%s: the initial item factors are not finite", who);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  SampleProfiles profiles;      // a refusal leaves the state held as it is
  TRY(profiles_upload(profiles, who, U, n, indptr, indices, ratings, nullptr, nullptr));

  mf_sgd_drop(h);
  MfSgdState& s = h->mfs;
  s.profiles = std::move(profiles);
  s.k = k;
  s.block = (size_t)U * k + (size_t)n * k + (size_t)U + (size_t)n + 1;
  if (int rc = s.P.alloc(who, "the factors, the biases and their optimiser state (float64)", 3 * s.block)) {
    mf_sgd_drop(h);
    return rc;
  }
  hipError_t e = hipMemset(s.P, 0, 3 * s.block * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(s.P, user_factors, (size_t)U * k * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s.P + (size_t)U * k, item_factors, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { mf_sgd_drop(h); return fail(-2, "%s: %s", who, hipGetErrorString(e)); }
  s.algo = algorithm; s.use_bias = use_bias; s.sgd = sgd_mode;
  s.lr = learning_rate; s.user_reg = user_reg; s.item_reg = item_reg; s.pos_reg = positive_reg; s.neg_reg = negative_reg;
  s.bias_reg = bias_reg; s.quota = negative_interactions_quota;
  s.b1_pow = s.b1; s.b2_pow = s.b2;      // (MatrixFactorization_Cython_Epoch.pyx:207-208)
  s.seed = seed; s.epoch = 0;
  s.ready = true;
  return 0;
}

// the samples of an epoch: a multiple of the batch size (:290, :617)
static int mf_sgd_per_epoch(ganmf_handle* h, const char* who, int64_t batch_size, int64_t* per) {
  if (batch_size < 1 || batch_size > GANMF_MF_SGD_MAX_BATCH)
    return fail(-1, "%s: batch_size must be in [1, %d]", who, GANMF_MF_SGD_MAX_BATCH);
  const int64_t base = h->mfs.algo == MF_SGD_BPR ? (int64_t)h->U : h->mfs.profiles.nnz;
  *per = (base / batch_size + 1) * batch_size;
  if (*per > SGD_MAX_SAMPLES) return fail(-1, "%s: more than 2^30 samples in one epoch", who);
  return 0;
}

// the list is on the device (t) and, for the levelled route, its ids on the host (checked by the caller)
static int mf_sgd_run_device(ganmf_handle* h, const char* who, SampleList& t, const int32_t* users, const int32_t* pos, const int32_t* neg,
                             int64_t n, int64_t batch_size, int route, int64_t* n_levels) {
  MfSgdState& s = h->mfs;
  const bool levelled = route != GANMF_MF_SGD_SEQUENTIAL;
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  if (s.terms.cap < (size_t)batch_size) {
    HIP_TRY(hipStreamSynchronize(h->st));
    TRY(s.terms.alloc(who, "the per-sample terms of a batch", (size_t)batch_size));
  }
  MfSgdP p{};
  mf_sgd_block(h, 0, &p.W, &p.H, &p.ub, &p.ib, &p.gb);
  mf_sgd_block(h, 1, &p.W0, &p.H0, &p.ub0, &p.ib0, &p.gb0);
  mf_sgd_block(h, 2, &p.W1, &p.H1, &p.ub1, &p.ib1, &p.gb1);
  p.k = s.k; p.algo = s.algo; p.use_bias = s.use_bias; p.sgd = s.sgd;
  p.lr = s.lr; p.user_reg = s.user_reg; p.pos_reg = s.pos_reg; p.neg_reg = s.neg_reg; p.bias_reg = s.bias_reg;
  p.gamma = s.gamma; p.b1 = s.b1; p.b2 = s.b2;
  p.users = t.users; p.pos = t.pos; p.neg = t.neg; p.rating = t.rating; p.terms = s.terms;
  const int64_t n_batches = (n + batch_size - 1) / batch_size;
  std::vector<int64_t> order, starts;      // levelled: list positions by (batch, level); every batch's level bounds, then its end
  std::vector<int64_t> batch_at((size_t)n_batches + 1, 0);      // where a batch's bounds begin in `starts`
  int64_t top = 0;
  if (levelled) {
    order.resize((size_t)n);
    LevelScheduler scheduler((int64_t)h->U + h->N);      // users, then items at base U: one table through every batch
    LevelSchedule sched;
    for (int64_t b = 0; b < n_batches; ++b) {
      const int64_t first = b * batch_size, count = std::min(batch_size, n - first);
      std::vector<LevelColumn> cols = {{users + first, 0, h->U}, {pos + first, h->U, h->N}};
      if (neg) cols.push_back({neg + first, h->U, h->N});
      const int64_t levels = scheduler.schedule(cols, count, sched);
      if (levels < 0) return fail(-2, "%s: the schedule met an id out of range", who);
      top = std::max(top, levels);
      batch_at[(size_t)b] = (int64_t)starts.size();
      for (int64_t l = 0; l < levels; ++l) starts.push_back(first + sched.level_start[(size_t)l]);
      for (int64_t q = 0; q < count; ++q) order[(size_t)(first + q)] = first + sched.order[(size_t)q];
    }
    batch_at[(size_t)n_batches] = (int64_t)starts.size();
    TRY(t.upload_order(who, h->st, order));
    p.order = t.order;
  }
  constexpr int per_wg = MF_SGD_THREADS / MF_SGD_WAVE;
  double b1p = s.b1_pow, b2p = s.b2_pow;
  for (int64_t b = 0; b < n_batches; ++b) {
    const int64_t first = b * batch_size, count = std::min(batch_size, n - first);
    GANMF_LAUNCH(mf_predict_kernel, dim3((unsigned)((count + per_wg - 1) / per_wg)), dim3(MF_SGD_THREADS), 0, h->st, p, (long long)first,
                 (long long)count);
    HIP_TRY(hipGetLastError());
    if (!levelled) {
      GANMF_LAUNCH(mf_update_kernel, dim3(1), dim3(MF_SGD_WAVE), 0, h->st, p, (long long)first, (long long)count, 0LL, 0LL, 1, 1, b1p, b2p);
      HIP_TRY(hipGetLastError());
    } else {
      for (int64_t q = batch_at[(size_t)b]; q < batch_at[(size_t)b + 1]; ++q) {
        const int64_t lf = starts[(size_t)q], le = q + 1 < batch_at[(size_t)b + 1] ? starts[(size_t)q + 1] : first + count;
        GANMF_LAUNCH(mf_update_kernel, dim3((unsigned)((le - lf + per_wg - 1) / per_wg)), dim3(MF_SGD_THREADS), 0, h->st, p,
                     (long long)first, (long long)count, (long long)lf, (long long)(le - lf), 0, q == batch_at[(size_t)b] ? 1 : 0, b1p, b2p);
        HIP_TRY(hipGetLastError());
      }
    }
    if (s.sgd == SGD_ADAM) {      // once per batch (:393-397, :699-703)
      b1p *= s.b1;
      b2p *= s.b2;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->st));      // (order leaves scope)
  s.b1_pow = b1p;
  s.b2_pow = b2p;
  if (n_levels) *n_levels = top;
  return 0;
}

int ganmf_mf_sgd_draw(ganmf_handle* h, int64_t epoch, int64_t n_epochs, int64_t batch_size, int32_t* users, int32_t* items,
                      int32_t* neg_items, double* ratings) {
  const char* who = "ganmf_mf_sgd_draw";
  if (!h || !users || !items) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_ready(h, who));
  const int algo = h->mfs.algo;
  if (algo == MF_SGD_BPR ? !neg_items : !ratings) return fail(-1, "%s: null argument", who);
  if (epoch < 0 || n_epochs < 0) return fail(-1, "%s: epoch and n_epochs must be >= 0", who);
  int64_t per = 0;
  TRY(mf_sgd_per_epoch(h, who, batch_size, &per));
  int64_t n = 0;
  TRY(sample_count(who, n_epochs, per, &n));
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  const MfSgdState& s = h->mfs;
  const bool rated = algo == MF_SGD_FUNK;
  SampleList t;
  TRY(t.alloc(who, n, rated));
  TRY(sample_draw(h, s.profiles, rated, s.quota, s.seed, epoch, per, n, t));
  return t.download(h->st, n, users, items, rated ? nullptr : neg_items, rated ? ratings : nullptr);
}

int ganmf_mf_sgd_run(ganmf_handle* h, const int32_t* users, const int32_t* items, const int32_t* neg_items, const double* ratings, int64_t n,
                     int64_t batch_size, int route, int64_t* n_levels) {
  const char* who = "ganmf_mf_sgd_run";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_ready(h, who));
  const bool bpr = h->mfs.algo == MF_SGD_BPR;
  if (n > 0 && (!users || !items || (bpr ? !neg_items : !ratings))) return fail(-1, "%s: null argument", who);
  TRY(sgd_route_ok(who, route));
  TRY(sample_n_ok(who, n));
  if (batch_size < 1 || batch_size > GANMF_MF_SGD_MAX_BATCH) return fail(-1, "%s: batch_size must be in [1, %d]", who, GANMF_MF_SGD_MAX_BATCH);
  TRY(sample_list_ok(h, who, users, items, neg_items, bpr ? nullptr : ratings, n));
  if (n_levels) *n_levels = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(h->dev));
  SampleList t;
  TRY(t.upload(who, h->st, n, users, items, neg_items, bpr ? nullptr : ratings));
  return mf_sgd_run_device(h, who, t, users, items, bpr ? neg_items : nullptr, n, batch_size, route, n_levels);
}

int ganmf_mf_sgd_epochs(ganmf_handle* h, int64_t n_epochs, int64_t batch_size, int route, int64_t* n_levels) {
  const char* who = "ganmf_mf_sgd_epochs";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_ready(h, who));
  TRY(sgd_route_ok(who, route));
  if (n_epochs < 0) return fail(-1, "%s: n_epochs must be >= 0", who);
  int64_t per = 0;
  TRY(mf_sgd_per_epoch(h, who, batch_size, &per));
  if (n_levels) *n_levels = 0;
  HIP_TRY(hipSetDevice(h->dev));
  const bool bpr = h->mfs.algo == MF_SGD_BPR, levelled = route != GANMF_MF_SGD_SEQUENTIAL;
  std::vector<int32_t> users, pos, neg;
  int64_t top = 0;
  for (int64_t e = 0; e < n_epochs; ++e) {
    SampleList t;
    TRY(t.alloc(who, per, !bpr));
    TRY(sample_draw(h, h->mfs.profiles, !bpr, h->mfs.quota, h->mfs.seed, h->mfs.epoch, per, per, t));
    if (levelled) TRY(t.ids_to_host(h->st, per, true, users, pos, neg));
    int64_t levels = 0;
    TRY(mf_sgd_run_device(h, who, t, users.data(), pos.data(), bpr ? neg.data() : nullptr, per, batch_size, route, &levels));
    top = std::max(top, levels);
    ++h->mfs.epoch;
  }
  if (n_levels) *n_levels = top;
  return 0;
}

int ganmf_mf_sgd_publish(ganmf_handle* h) {
  const char* who = "ganmf_mf_sgd_publish";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_ready(h, who));
  const MfSgdState& s = h->mfs;
  HIP_TRY(hipSetDevice(h->dev));
  MfPublishP p{};
  double *W, *H, *ub, *ib, *gb;
  mf_sgd_block(h, 0, &W, &H, &ub, &ib, &gb);
  p.W = W; p.H = H; p.ub = ub; p.ib = ib; p.gb = gb;
  p.Ue = h->Ue.p; p.V = h->V.p;
  p.n_users = h->U; p.n_items = h->N; p.k = s.k; p.use_bias = s.use_bias; p.ld = h->ldk;
  const long long cells = ((long long)h->U + h->N) * h->k;
  ++h->param_version;
  GANMF_LAUNCH(mf_publish_kernel, dim3((unsigned)((cells + MF_SGD_THREADS - 1) / MF_SGD_THREADS)), dim3(MF_SGD_THREADS), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->st));
  return 0;
}

int ganmf_mf_sgd_get_state(ganmf_handle* h, double* params, double* state0, double* state1, double* beta_powers, int64_t* epoch) {
  const char* who = "ganmf_mf_sgd_get_state";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_ready(h, who));
  const MfSgdState& s = h->mfs;
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  double* out[3] = {params, state0, state1};
  for (int b = 0; b < 3; ++b)
    if (out[b]) HIP_TRY(hipMemcpy(out[b], s.P + (size_t)b * s.block, s.block * sizeof(double), hipMemcpyDeviceToHost));
  if (beta_powers) { beta_powers[0] = s.b1_pow; beta_powers[1] = s.b2_pow; }
  if (epoch) *epoch = s.epoch;
  return 0;
}

int ganmf_mf_sgd_set_state(ganmf_handle* h, const double* params, const double* state0, const double* state1, const double* beta_powers,
                           int64_t epoch) {
  const char* who = "ganmf_mf_sgd_set_state";
  if (!h) return fail(-1, "%s: null argument", who);
  TRY(mf_sgd_ready(h, who));
  MfSgdState& s = h->mfs;
  if (epoch < -1) return fail(-1, "%s: epoch must be >= 0, or -1 to keep the counter", who);
  if (beta_powers && !(std::isfinite(beta_powers[0]) && std::isfinite(beta_powers[1]))) return fail(-1, "%s: the beta powers must be finite", who);
  const double* in[3] = {params, state0, state1};
  for (int b = 0; b < 3; ++b)
    if (in[b])
      for (size_t q = 0; q < s.block; ++q)
        if (!std::isfinite(in[b][q])) return fail(-1, "%s: block %d holds a value that is not finite", who, b);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  for (int b = 0; b < 3; ++b)
    if (in[b]) HIP_TRY(hipMemcpy(s.P + (size_t)b * s.block, in[b], s.block * sizeof(double), hipMemcpyHostToDevice));
  if (beta_powers) { s.b1_pow = beta_powers[0]; s.b2_pow = beta_powers[1]; }
  if (epoch >= 0) s.epoch = epoch;
  return 0;
}
