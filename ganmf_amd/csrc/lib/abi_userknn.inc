// abi_userknn.inc -- C ABI: user-based nearest neighbours on a GANMF_MODEL_ITEMSIM handle: ganmf_userknn_fit / ganmf_userknn_get /
// ganmf_set_user_similarity, and the product behind scores_device while a user matrix is held (userknn_rows.hpp).  The handle holds
// one similarity matrix; knn_user says which (handle.inc).  The fit is ganmf_itemknn_fit's with the sides of the URM exchanged.
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

static int usersim_product(ganmf_handle* h, const int* ids_dev, int64_t n, int W, int ldw) {
  UserKnnScoreP p{};
  const AlsSide& s = h->als[0];
  p.r_indptr = s.indptr; p.r_items = s.indices; p.r_val = s.conf;
  p.w_indptr = h->knn.indptr; p.w_nbr = h->knn.indices; p.w_val = h->knn.val;
  p.ids = ids_dev; p.n = (int)n; p.n_items = W; p.out = h->sc_out; p.ldo = ldw;
  p.acc_lds = W <= KNN_SCORE_LDS ? 1 : 0;
  const size_t shmem = p.acc_lds ? (size_t)W * sizeof(float) : 0;
  TRY(allow_lds((const void*)userknn_score_kernel, shmem));
  // every scored row reads its neighbours' profiles: about nnz(W) / U rows of nnz(R) / U entries each
  const double per_row = (double)std::max<int64_t>(h->knn_nnz, 0) / std::max(h->U, 1) * ((double)s.nnz / std::max(h->U, 1));
  Scope sc(h, T_KNN_SCORE, 2.0 * n * per_row, 8.0 * n * per_row + 4.0 * n * W);
  GANMF_LAUNCH(userknn_score_kernel, dim3((unsigned)n), dim3(KNN_THREADS), shmem, h->st, p);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the three arrays of a [n_users, n_users] matrix by row into the handle: dropped first, valid last
static int usersim_hold(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const float* data, int n) {
  const int64_t nnz = indptr[n];
  TRY(h->knn.upload(indptr, indices, n, n));
  TRY(h->knn.upload_values(h->knn.val, data));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->knn_user = 1;
  h->knn_nnz = nnz;
  return 0;
}

int ganmf_set_user_similarity(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_users) {
  const char* who = "ganmf_set_user_similarity";
  if (!h || !indptr) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (n_users != h->U) return fail(-1, "%s: the handle has %d users, given %lld", who, h->U, (long long)n_users);
  TRY(check_csr(who, indptr, indices, n_users, n_users, false, false));
  const int64_t nnz = indptr[n_users];
  if (nnz > 0 && !data) return fail(-1, "%s: null argument", who);
  for (int64_t j = 0; j < nnz; ++j)
    if (!std::isfinite(data[j])) return fail(-1, "%s: weight %lld is not finite", who, (long long)j);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  itemsim_drop(h);
  return usersim_hold(h, indptr, indices, data, (int)n_users);
}

int ganmf_userknn_get(ganmf_handle* h, int64_t* indptr, int32_t* indices, float* data) {
  const char* who = "ganmf_userknn_get";
  if (!h || !indptr) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (h->knn_nnz < 0) return fail(-1, "%s: the handle holds no user similarity matrix", who);
  if (!h->knn_user) return fail(-1, "%s: the handle holds an item similarity matrix (ganmf_itemknn_get reads it)", who);
  if (h->knn_nnz > 0 && (!indices || !data)) return fail(-1, "%s: null argument", who);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  HIP_TRY(hipMemcpy(indptr, h->knn.indptr, (size_t)(h->U + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (h->knn_nnz > 0) {
    HIP_TRY(hipMemcpy(indices, h->knn.indices, (size_t)h->knn_nnz * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data, h->knn.val, (size_t)h->knn_nnz * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}

int ganmf_userknn_fit(ganmf_handle* h, int kind, int32_t topk, float shrink, float p0, float p1, const float* den_a, const float* den_b,
                      int64_t* nnz_out) {
  const char* who = "ganmf_userknn_fit";
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
  const int n = h->U, k = std::min<int>(topk, n);
  for (int j = 0; j < n && kind <= KNN_TVERSKY; ++j)
    if (!std::isfinite(den_a[j]) || (kind == KNN_PRODUCT && !std::isfinite(den_b[j]))) return fail(-1, "%s: denominator term %d is not finite", who, j);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  itemsim_drop(h);
  SimFloats den;
  SimPicks t;
  SimCsr C;      // the result by target user: column i of W_sparse
  const AlsSide& s = h->als[0];
  const SimRowPlan plan = itemsim_row_plan(n);
  KnnFitP p{};
  p.kind = kind; p.s = (float)((double)shrink + 1e-6); p.shrink = shrink; p.p0 = p0; p.p1 = p1;
  if (kind <= KNN_TVERSKY) TRY(upload_floats(den.a, den_a, n));
  if (kind == KNN_PRODUCT) TRY(upload_floats(den.b, den_b, n));
  p.den_a = den.a; p.den_b = den.b;
  TRY(t.alloc(n, k, plan.row_floats()));
  const size_t shmem = itemsim_row_args(h, 0, n, h->N, k, plan, t, &p);      // the rows of side 0 compared over the items
  TRY(allow_lds((const void*)itemknn_fit_kernel, shmem));
  {
    Scope sc(h, T_KNN_FIT, 2.0 * n * (double)s.nnz, 8.0 * n * (double)s.nnz);
    GANMF_LAUNCH(itemknn_fit_kernel, dim3(plan.grid), dim3(KNN_THREADS), shmem, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  TRY(itemsim_compact(h, who, n, t, k, k, C));
  HIP_TRY(hipStreamSynchronize(h->st));
  // ---- by target user -> by row, on the host: a stable counting sort by the stored neighbour.  Columns are visited in ascending
  // order, so every row ascends.  (At most n * k entries; a row has no bound of its own.) ----
  const size_t nnz = (size_t)C.nnz;
  std::vector<int64_t> cp((size_t)n + 1), rp((size_t)n + 1, 0), at;
  std::vector<int> cj(std::max<size_t>(nnz, 1)), ri(std::max<size_t>(nnz, 1));
  std::vector<float> cv(std::max<size_t>(nnz, 1)), rv(std::max<size_t>(nnz, 1));
  HIP_TRY(hipMemcpy(cp.data(), C.indptr, ((size_t)n + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (nnz) {
    HIP_TRY(hipMemcpy(cj.data(), C.indices, nnz * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cv.data(), C.val, nnz * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (cp[0] != 0 || cp[(size_t)n] != (int64_t)nnz) return fail(-2, "%s: the compact matrix came back with a bad indptr", who);
  for (size_t q = 0; q < nnz; ++q) {
    if (cj[q] < 0 || cj[q] >= n) return fail(-2, "%s: the compact matrix came back with neighbour %d of %d users", who, cj[q], n);
    ++rp[(size_t)cj[q] + 1];
  }
  for (int j = 0; j < n; ++j) rp[(size_t)j + 1] += rp[(size_t)j];
  at.assign(rp.begin(), rp.end() - 1);
  for (int i = 0; i < n; ++i)
    for (int64_t q = cp[(size_t)i]; q < cp[(size_t)i + 1]; ++q) {
      const int64_t o = at[(size_t)cj[(size_t)q]]++;
      ri[(size_t)o] = i; rv[(size_t)o] = cv[(size_t)q];
    }
  TRY(usersim_hold(h, rp.data(), ri.data(), rv.data(), n));
  *nnz_out = (int64_t)nnz;
  return 0;
}
