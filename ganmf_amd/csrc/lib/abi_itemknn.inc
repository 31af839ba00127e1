// abi_itemknn.inc -- C ABI: item-based nearest neighbours on a GANMF_MODEL_ITEMSIM handle: ganmf_itemknn_fit / ganmf_itemknn_get /
// ganmf_set_item_similarity, and the second score source behind scores_device (itemknn_rows.hpp)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static int itemsim_handle(ganmf_handle* h, const char* who) {
  TRY(not_cfgan(h, who));
  if (h->cfg.model != GANMF_MODEL_ITEMSIM) return fail(-1, "%s: needs a GANMF_MODEL_ITEMSIM handle", who);
  if (h->has_comm && h->cfg.world_size > 1) return fail(-1, "%s: single-GPU entry", who);
  return 0;
}
static int itemsim_side(ganmf_handle* h, const char* who, int side) {
  const AlsSide& s = h->als[side];
  if (!s.indptr) return fail(-1, "%s: ganmf_als_set_confidence has not been called for side %d (the weighted URM%s)", who, side, side ? ", by item" : "");
  if (!s.canonical)
    return fail(-1, "%s: side %d has a row whose columns do not ascend or repeat; this model needs the canonical form (sorted indices, duplicates summed)", who, side);
  return 0;
}

static int itemsim_ready(ganmf_handle* h, const char* who, int transposed) {
  if (h->cfg.model != GANMF_MODEL_ITEMSIM) return 0;
  if (transposed) return fail(-1, "%s: transposed = 1 is not defined on a GANMF_MODEL_ITEMSIM handle (its scores are URM[users] . W)", who);
  TRY(itemsim_side(h, who, 0));
  if (h->knn_nnz < 0) return fail(-1, "%s: the handle holds no item similarity matrix (ganmf_itemknn_fit or ganmf_set_item_similarity)", who);
  return 0;
}

static int usersim_product(ganmf_handle* h, const int* ids_dev, int64_t n, int W, int ldw);      // (abi_userknn.inc)

static int itemsim_product(ganmf_handle* h, const int* ids_dev, int64_t n, int W, int ldw) {
  if (h->knn_user) return usersim_product(h, ids_dev, n, W, ldw);      // a held user matrix: W[users] . URM
  KnnScoreP p{};
  const AlsSide& s = h->als[0];
  p.r_indptr = s.indptr; p.r_items = s.indices; p.r_val = s.conf;
  p.w_indptr = h->knn.indptr; p.w_nbr = h->knn.indices; p.w_val = h->knn.val;
  p.ids = ids_dev; p.n = (int)n; p.n_items = W; p.out = h->sc_out; p.ldo = ldw;
  const bool lds = W <= KNN_SCORE_LDS;
  const int G = !lds ? 4 : 8 * W <= KNN_SCORE_GROUP ? 8 : 4 * W <= KNN_SCORE_GROUP ? 4 : 2 * W <= KNN_SCORE_GROUP ? 2 : 1;
  if (!lds) {      // dense profiles in global memory, whole groups of rows
    const size_t rows = (size_t)round_up((int)n, 8);
    TRY(h->knn_dense.grow(h->st, rows * ldw, false));
    HIP_TRY(hipMemsetAsync(h->knn_dense, 0, rows * ldw * sizeof(float), h->st));
    p.dense = h->knn_dense; p.ldd = ldw;
    GANMF_LAUNCH(itemknn_densify_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  const unsigned groups = (unsigned)((n + G - 1) / G);
  const unsigned chunks_max = (unsigned)((W + KNN_THREADS - 1) / KNN_THREADS);
  const unsigned chunks = std::max(1u, std::min(chunks_max, (1024u + groups - 1) / groups));      // about a thousand workgroups
  const size_t shmem = lds ? (size_t)G * W * sizeof(float) : 0;
  const double nnz_w = (double)std::max<int64_t>(h->knn_nnz, 0);
  Scope sc(h, T_KNN_SCORE, 2.0 * n * nnz_w, 8.0 * nnz_w * groups + 4.0 * n * W);
  switch (lds ? G : 0) {
    case 8:
      TRY(allow_lds((const void*)itemknn_score_kernel<8, true>, shmem));
      GANMF_LAUNCH((itemknn_score_kernel<8, true>), dim3(groups, chunks), dim3(KNN_THREADS), shmem, h->st, p);
      break;
    case 4:
      TRY(allow_lds((const void*)itemknn_score_kernel<4, true>, shmem));
      GANMF_LAUNCH((itemknn_score_kernel<4, true>), dim3(groups, chunks), dim3(KNN_THREADS), shmem, h->st, p);
      break;
    case 2:
      TRY(allow_lds((const void*)itemknn_score_kernel<2, true>, shmem));
      GANMF_LAUNCH((itemknn_score_kernel<2, true>), dim3(groups, chunks), dim3(KNN_THREADS), shmem, h->st, p);
      break;
    case 1:
      TRY(allow_lds((const void*)itemknn_score_kernel<1, true>, shmem));
      GANMF_LAUNCH((itemknn_score_kernel<1, true>), dim3(groups, chunks), dim3(KNN_THREADS), shmem, h->st, p);
      break;
    default:
      GANMF_LAUNCH((itemknn_score_kernel<4, false>), dim3(groups, chunks), dim3(KNN_THREADS), 0, h->st, p);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// The held matrix is dropped.  Every fit and upload drops first and sets h->knn_nnz LAST, behind its final synchronise: any failure
// in between leaves "no matrix" (knn_nnz < 0) and an empty holder.
static void itemsim_drop(ganmf_handle* h) {
  h->knn.drop();
  h->knn_nnz = -1; h->knn_user = 0;
}

// ---- what the fits share (ganmf_itemknn_fit, ganmf_p3_fit, ganmf_slim_bpr_finish) --------------------------------------------------
// The picks of one selection pass -- [n, k] ids and values in descending order of value, [n] counts -- and the private rows of the
// global route, released on every way out.
struct SimPicks {
  DevBuf<int> idx, cnt;
  DevBuf<float> val, row;
  int alloc(int n, int k, size_t row_floats) {
    if (row_floats) TRY(row.alloc(row_floats, false));
    TRY(idx.alloc((size_t)n * k, false));
    TRY(val.alloc((size_t)n * k, false));
    TRY(cnt.alloc((size_t)n, false));
    return 0;
  }
};
// host vectors of a fit on the device, released on every way out (the compact matrix between two passes is a SimCsr, handle.inc)
struct SimFloats { DevBuf<float> a, b; };
static int upload_floats(DevBuf<float>& dst, const float* src, int n) {
  TRY(dst.alloc((size_t)n, false));
  HIP_TRY(hipMemcpy(dst, src, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

// Where a workgroup keeps its dense row of n floats: in LDS up to KNN_ROW_LDS items, one workgroup per item up to 8192 of them; above,
// a private row in global memory ([grid, ld_row] floats), at most 512 workgroups.
struct SimRowPlan {
  int row_lds;
  unsigned grid;
  long long ld_row;
  size_t row_floats() const { return row_lds ? 0 : (size_t)grid * ld_row; }
};
static SimRowPlan itemsim_row_plan(int n) {
  SimRowPlan r{};
  r.row_lds = n <= KNN_ROW_LDS ? 1 : 0;
  r.grid = (unsigned)std::min(n, r.row_lds ? 8192 : 512);
  r.ld_row = r.row_lds ? 0 : round_up(n, LD_ALIGN);
  return r;
}

// What the two row builders read (SimRowP: the side whose n rows are compared over their m columns -- side 1 with (N, U) for the item
// models, side 0 with (U, N) for ganmf_userknn_fit --, the slab, the plan's row, the picks); returns the dynamic LDS of their launch:
// the slab, and behind it the row where the plan keeps it in LDS.
static size_t itemsim_row_args(ganmf_handle* h, int side, int n, int m, int k, const SimRowPlan& plan, const SimPicks& t, SimRowP* p) {
  const AlsSide& s = h->als[side];
  p->c_indptr = s.indptr; p->c_users = s.indices; p->c_val = s.conf;
  p->n_items = n; p->n_users = m; p->topk = k;
  p->slab = std::min(KNN_SLAB, round_up(m, 64));
  p->row_lds = plan.row_lds; p->row_glob = t.row; p->ld_row = plan.ld_row;
  p->out_idx = t.idx; p->out_val = t.val; p->out_cnt = t.cnt;
  return ((size_t)p->slab + (plan.row_lds ? (size_t)n : 0)) * sizeof(float);
}

// [n] counts from the device (enqueued behind the kernel that wrote them) to an indptr on the host
static int itemsim_indptr(ganmf_handle* h, const char* who, const int* cnt_dev, int n, long long most, std::vector<int64_t>& ip) {
  std::vector<int> cnt((size_t)n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), cnt_dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  ip.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (cnt[(size_t)i] < 0 || cnt[(size_t)i] > most) return fail(-2, "%s: item %d reports %d entries of at most %lld", who, i, cnt[(size_t)i], most);
    ip[(size_t)i + 1] = ip[(size_t)i] + cnt[(size_t)i];
  }
  return 0;
}

// the three arrays of a compact [n, n] matrix (one element where it is empty), its indptr uploaded
static int itemsim_alloc(const int64_t* ip, int n, SimCsr& m) {
  TRY(m.upload(ip, nullptr, n, n));
  return m.upload_values(m.val, (const float*)nullptr);
}

// The picks of a pass (k per item of the n in their layout, at most `most` stored) to a compact [n, n] matrix, ids ascending inside an
// item: the counts read back, the indptr formed and checked, the matrix allocated, itemknn_pack_kernel.  Into temporaries between two
// passes, into the handle for the result.
static int itemsim_compact(ganmf_handle* h, const char* who, int n, const SimPicks& t, int k, long long most, SimCsr& m) {
  std::vector<int64_t> ip;
  TRY(itemsim_indptr(h, who, t.cnt, n, most, ip));
  TRY(itemsim_alloc(ip.data(), n, m));
  Scope sc(h, T_KNN_PACK, 0.0, 16.0 * (double)m.nnz);
  GANMF_LAUNCH(itemknn_pack_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, h->st, (const int*)t.idx, (const float*)t.val,
               (const int*)t.cnt, k, (const long long*)m.indptr, m.indices.get(), m.val.get());
  HIP_TRY(hipGetLastError());
  return 0;
}

// The column pass (p3_columns_kernel): the ck largest non-zeros of every column of R, bit copies, into the picks.  The dense column
// lives where the plan puts a row, and the grid is the plan's: min(n, 8192) workgroups with the column in LDS, at most 512 above.
static int itemsim_columns(ganmf_handle* h, int n, const SimCsr& R, int ck, const SimRowPlan& plan, const SimPicks& t) {
  P3ColP p{};
  p.r_indptr = R.indptr; p.r_idx = R.indices; p.r_val = R.val;
  p.n_items = n; p.topk = ck;
  p.row_lds = plan.row_lds; p.row_glob = t.row; p.ld_row = plan.ld_row;
  p.out_idx = t.idx; p.out_val = t.val; p.out_cnt = t.cnt;
  const size_t shmem = plan.row_lds ? (size_t)n * sizeof(float) : 0;
  TRY(allow_lds((const void*)p3_columns_kernel, shmem));
  Scope sc(h, T_P3_COLUMNS, 0.0, 16.0 * (double)n * n);
  GANMF_LAUNCH(p3_columns_kernel, dim3(plan.grid), dim3(KNN_THREADS), shmem, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

int ganmf_set_item_similarity(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_items) {
  const char* who = "ganmf_set_item_similarity";
  if (!h || !indptr) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (n_items != h->N) return fail(-1, "%s: the handle has %d items, given %lld", who, h->N, (long long)n_items);
  TRY(check_csr(who, indptr, indices, n_items, n_items, false, false));
  const int64_t nnz = indptr[n_items];
  if (nnz > 0 && !data) return fail(-1, "%s: null argument", who);
  for (int64_t j = 0; j < nnz; ++j)
    if (!std::isfinite(data[j])) return fail(-1, "%s: weight %lld is not finite", who, (long long)j);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  itemsim_drop(h);
  TRY(h->knn.upload(indptr, indices, n_items, n_items));
  TRY(h->knn.upload_values(h->knn.val, data));
  h->knn_nnz = nnz;
  return 0;
}

int ganmf_itemknn_get(ganmf_handle* h, int64_t* indptr, int32_t* indices, float* data) {
  const char* who = "ganmf_itemknn_get";
  if (!h || !indptr) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (h->knn_nnz < 0) return fail(-1, "%s: the handle holds no item similarity matrix", who);
  if (h->knn_user) return fail(-1, "%s: the handle holds a user similarity matrix (ganmf_userknn_get reads it)", who);
  if (h->knn_nnz > 0 && (!indices || !data)) return fail(-1, "%s: null argument", who);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  HIP_TRY(hipMemcpy(indptr, h->knn.indptr, (size_t)(h->N + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (h->knn_nnz > 0) {
    HIP_TRY(hipMemcpy(indices, h->knn.indices, (size_t)h->knn_nnz * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data, h->knn.val, (size_t)h->knn_nnz * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}

static_assert(KNN_MAX_TOPK == GANMF_ITEMKNN_MAX_TOPK, "top-k limit of the kernels and of the header");
static_assert(KNN_PRODUCT == GANMF_ITEMKNN_PRODUCT && KNN_RAW == GANMF_ITEMKNN_RAW, "similarity kinds of the kernels and of the header");

int ganmf_itemknn_fit(ganmf_handle* h, int kind, int32_t topk, float shrink, float p0, float p1, const float* den_a, const float* den_b,
                      int64_t* nnz_out) {
  const char* who = "ganmf_itemknn_fit";
  if (!h || !nnz_out) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (kind < 0 || kind >= KNN_KINDS) return fail(-1, "%s: unknown similarity kind %d", who, kind);
  if (topk < 1 || topk > GANMF_ITEMKNN_MAX_TOPK) return fail(-1, "%s: topk %d out of range [1,%d] (GANMF_ITEMKNN_MAX_TOPK)", who, topk, GANMF_ITEMKNN_MAX_TOPK);
  if (!(shrink >= 0.f) || !std::isfinite(shrink)) return fail(-1, "%s: shrink must be finite and >= 0", who);
  if (kind == KNN_SHRINK_ONLY && shrink == 0.f) return fail(-1, "%s: GANMF_ITEMKNN_SHRINK_ONLY divides by shrink, which is 0", who);
  if (kind == KNN_TVERSKY && (!std::isfinite(p0) || !std::isfinite(p1))) return fail(-1, "%s: the Tversky coefficients are not finite", who);
  if (kind <= KNN_TVERSKY && !den_a) return fail(-1, "%s: kind %d needs den_a", who, kind);
  if (kind == KNN_PRODUCT && !den_b) return fail(-1, "%s: kind %d needs den_b", who, kind);
  TRY(itemsim_side(h, who, 0));
  TRY(itemsim_side(h, who, 1));
  const int n = h->N, k = std::min<int>(topk, n);
  for (int j = 0; j < n && kind <= KNN_TVERSKY; ++j)
    if (!std::isfinite(den_a[j]) || (kind == KNN_PRODUCT && !std::isfinite(den_b[j]))) return fail(-1, "%s: denominator term %d is not finite", who, j);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  itemsim_drop(h);
  SimFloats den;
  SimPicks t;
  const AlsSide& s = h->als[1];
  const SimRowPlan plan = itemsim_row_plan(n);
  KnnFitP p{};
  p.kind = kind; p.s = (float)((double)shrink + 1e-6); p.shrink = shrink; p.p0 = p0; p.p1 = p1;
  if (kind <= KNN_TVERSKY) TRY(upload_floats(den.a, den_a, n));
  if (kind == KNN_PRODUCT) TRY(upload_floats(den.b, den_b, n));
  p.den_a = den.a; p.den_b = den.b;
  TRY(t.alloc(n, k, plan.row_floats()));
  const size_t shmem = itemsim_row_args(h, 1, n, h->U, k, plan, t, &p);
  TRY(allow_lds((const void*)itemknn_fit_kernel, shmem));
  {      // every workgroup walks the whole matrix once per slab of its item
    Scope sc(h, T_KNN_FIT, 2.0 * n * (double)s.nnz, 8.0 * n * (double)s.nnz);
    GANMF_LAUNCH(itemknn_fit_kernel, dim3(plan.grid), dim3(KNN_THREADS), shmem, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  TRY(itemsim_compact(h, who, n, t, k, k, h->knn));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->knn_nnz = h->knn.nnz;
  *nnz_out = h->knn.nnz;
  return 0;
}
