// sgd_train.inc -- what the SGD trainers (abi_slim.inc, abi_mf_sgd.inc) share on the host: the profiles on the
// device, the sample list with its draw, its checks and its copies, and the level order (counter_draw.hpp, level_sched.hpp).
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static_assert(SGD_PLAIN == GANMF_SLIM_SGD && SGD_ADAGRAD == GANMF_SLIM_ADAGRAD && SGD_RMSPROP == GANMF_SLIM_RMSPROP &&
              SGD_ADAM == GANMF_SLIM_ADAM, "sgd modes of the kernels and of the header");
static_assert(GANMF_SLIM_AUTO == GANMF_MF_SGD_AUTO && GANMF_SLIM_SEQUENTIAL == GANMF_MF_SGD_SEQUENTIAL &&
              GANMF_SLIM_LEVELLED == GANMF_MF_SGD_LEVELLED, "one set of routes");
static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "indptr, order and id words");

constexpr int64_t SGD_MAX_SAMPLES = (int64_t)1 << 30;

// ---- the profiles -----------------------------------------------------------------------------------------------------------------
static void profiles_drop(SampleProfiles& pr) { pr = SampleProfiles(); }

// into an object that holds nothing, from host CSR (h_indptr != null; ratings optional) or from the device CSR (dev_indptr, dev_items)
static int profiles_upload(SampleProfiles& pr, const char* who, int n_users, int n_items, const int64_t* h_indptr, const int32_t* h_indices,
                           const double* h_ratings, const long long* dev_indptr, const int* dev_items) {
  const bool from_device = !h_indptr;
  std::vector<int64_t> copied;
  if (from_device) {
    copied.resize((size_t)n_users + 1);
    HIP_TRY(hipMemcpy(copied.data(), dev_indptr, copied.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    h_indptr = copied.data();
  }
  std::vector<int> users;
  for (int u = 0; u < n_users; ++u) {
    const int64_t len = h_indptr[(size_t)u + 1] - h_indptr[(size_t)u];
    if (len > 0 && len < n_items) users.push_back(u);
  }
  if (users.empty()) return fail(-1, "%s: no user has a profile that is neither empty nor full: there is nothing to sample", who);
  int rc = pr.upload(h_indptr, from_device ? dev_items : h_indices, n_users, n_items, from_device, who, "the profiles");
  if (!rc && h_ratings) rc = pr.upload_values(pr.ratings, h_ratings, false, who, "the profiles");
  if (!rc) rc = pr.eligible.alloc(who, "the eligible users", users.size());
  if (!rc) {
    const hipError_t e = hipMemcpy(pr.eligible, users.data(), users.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(-2, "%s: %s", who, hipGetErrorString(e));
  }
  if (rc) { profiles_drop(pr); return rc; }
  pr.n_eligible = (int)users.size();
  return 0;
}

// ---- the sample list on the device --------------------------------------------------------------------------------------------------
struct SampleList {
  DevBuf<int> users, pos, neg;      // neg: the BPR trainers'
  DevBuf<double> rating;            // FunkSVD's
  DevBuf<double> pows;              // SLIM-BPR under Adam: the beta powers of every sample
  DevBuf<long long> order;          // the levelled route: list positions sorted by level

  int alloc(const char* who, int64_t n, bool rated) {
    TRY(users.alloc(who, "the samples", (size_t)n));
    TRY(pos.alloc(who, "the samples", (size_t)n));
    if (rated) TRY(rating.alloc(who, "the samples", (size_t)n));
    else TRY(neg.alloc(who, "the samples", (size_t)n));
    return 0;
  }
  // host arrays in (h_rating != null: a rated list, else h_neg); done when it returns: the caller's arrays may change
  int upload(const char* who, hipStream_t st, int64_t n, const int32_t* h_users, const int32_t* h_pos, const int32_t* h_neg,
             const double* h_rating) {
    TRY(alloc(who, n, h_rating != nullptr));
    HIP_TRY(hipMemcpyAsync(users, h_users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(pos, h_pos, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    if (h_rating) HIP_TRY(hipMemcpyAsync(rating, h_rating, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpyAsync(neg, h_neg, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  // host arrays out: a null pointer skips its column
  int download(hipStream_t st, int64_t n, int32_t* h_users, int32_t* h_pos, int32_t* h_neg, double* h_rating) const {
    if (h_users) HIP_TRY(hipMemcpyAsync(h_users, users, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_pos) HIP_TRY(hipMemcpyAsync(h_pos, pos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_neg) HIP_TRY(hipMemcpyAsync(h_neg, neg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (h_rating) HIP_TRY(hipMemcpyAsync(h_rating, rating, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  // the one copy back of a drawn list: the ids the schedule is formed from (with_users: the user column is a key too)
  int ids_to_host(hipStream_t st, int64_t n, bool with_users, std::vector<int32_t>& h_users, std::vector<int32_t>& h_pos,
                  std::vector<int32_t>& h_neg) const {
    if (with_users) h_users.resize((size_t)n);
    h_pos.resize((size_t)n);
    if (neg) h_neg.resize((size_t)n);
    return download(st, n, with_users ? h_users.data() : nullptr, h_pos.data(), neg ? h_neg.data() : nullptr, nullptr);
  }
  // enqueued: `sorted` has to live until the stream is synchronised
  int upload_order(const char* who, hipStream_t st, const std::vector<int64_t>& sorted) {
    TRY(order.alloc(who, "the level order", sorted.size()));
    HIP_TRY(hipMemcpyAsync(order, sorted.data(), sorted.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    return 0;
  }
};

// the samples of n_epochs epochs of `per` each; the cap of one call
static int sample_count(const char* who, int64_t n_epochs, int64_t per, int64_t* n) {
  if (n_epochs > SGD_MAX_SAMPLES / per) return fail(-1, "%s: more than 2^30 samples in one call", who);
  *n = n_epochs * per;
  return 0;
}

// n samples of the epochs [epoch, ...) with `per` samples each into the (allocated) list: one launch
static int sample_draw(ganmf_handle* h, const SampleProfiles& pr, bool rated, double quota, uint64_t seed, int64_t epoch, int64_t per,
                       int64_t n, SampleList& t) {
  DrawP p{};
  p.indptr = pr.indptr; p.items = pr.indices; p.ratings = pr.ratings; p.eligible = pr.eligible;
  p.n_users = h->U; p.n_items = h->N; p.n_eligible = pr.n_eligible; p.rated = rated ? 1 : 0; p.quota = quota;
  p.seed = seed; p.epoch0 = epoch; p.per_epoch = per; p.n = n;
  p.users = t.users; p.pos = t.pos; p.neg = t.neg; p.rating = t.rating;
  const unsigned blocks = (unsigned)((n + DRAW_THREADS - 1) / DRAW_THREADS);
  GANMF_LAUNCH(draw_kernel, dim3(blocks), dim3(DRAW_THREADS), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// an injected list: its length, then every id (ratings != null: a rated list, else neg is the third column)
static int sample_n_ok(const char* who, int64_t n) {
  if (n < 0 || n > SGD_MAX_SAMPLES) return fail(-1, "%s: n out of range", who);
  return 0;
}

static int sample_list_ok(ganmf_handle* h, const char* who, const int32_t* users, const int32_t* pos, const int32_t* neg,
                          const double* ratings, int64_t n) {
  for (int64_t q = 0; q < n; ++q) {
    if (users[q] < 0 || users[q] >= h->U) return fail(-1, "%s: sample %lld names user %d of %d", who, (long long)q, users[q], h->U);
    if (pos[q] < 0 || pos[q] >= h->N) return fail(-1, "%s: sample %lld names item %d of %d", who, (long long)q, pos[q], h->N);
    if (ratings) {
      if (!std::isfinite(ratings[q])) return fail(-1, "%s: sample %lld has a rating that is not finite", who, (long long)q);
      continue;
    }
    if (neg[q] < 0 || neg[q] >= h->N) return fail(-1, "%s: sample %lld names item %d of %d", who, (long long)q, neg[q], h->N);
    if (pos[q] == neg[q]) return fail(-1, "%s: sample %lld has the same positive and negative item %d", who, (long long)q, pos[q]);
  }
  return 0;
}

static int sgd_route_ok(const char* who, int route) {
  if (route != GANMF_SLIM_AUTO && route != GANMF_SLIM_SEQUENTIAL && route != GANMF_SLIM_LEVELLED)
    return fail(-1, "%s: unknown route %d", who, route);
  return 0;
}
