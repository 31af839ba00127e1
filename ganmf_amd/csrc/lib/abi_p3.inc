// abi_p3.inc -- C ABI: the graph-based item models P3alpha / RP3beta on a GANMF_MODEL_ITEMSIM handle: ganmf_p3_fit (p3_rows.hpp).  The
// result is held like ganmf_itemknn_fit's: ganmf_itemknn_get, ganmf_set_item_similarity and the scores read it unchanged.
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

int ganmf_p3_fit(ganmf_handle* h, int32_t topk, int32_t col_topk, int normalize, const float* row_scale, const float* col_scale,
                 int64_t* nnz_out) {
  const char* who = "ganmf_p3_fit";
  if (!h || !nnz_out || !row_scale) return fail(-1, "%s: null argument", who);
  TRY(itemsim_handle(h, who));
  if (topk < 1 || topk > GANMF_ITEMKNN_MAX_TOPK) return fail(-1, "%s: topk %d out of range [1,%d] (GANMF_ITEMKNN_MAX_TOPK)", who, topk, GANMF_ITEMKNN_MAX_TOPK);
  if (col_topk < 0 || col_topk > GANMF_ITEMKNN_MAX_TOPK)
    return fail(-1, "%s: col_topk %d out of range [0,%d] (GANMF_ITEMKNN_MAX_TOPK)", who, col_topk, GANMF_ITEMKNN_MAX_TOPK);
  TRY(itemsim_side(h, who, 0));
  TRY(itemsim_side(h, who, 1));
  const int n = h->N, k = std::min<int>(topk, n), ck = std::min<int>(col_topk, n);
  for (int j = 0; j < n; ++j) {
    if (!std::isfinite(row_scale[j]) || row_scale[j] < 0.f) return fail(-1, "%s: row_scale[%d] is negative or not finite", who, j);
    if (col_scale && (!std::isfinite(col_scale[j]) || col_scale[j] < 0.f)) return fail(-1, "%s: col_scale[%d] is negative or not finite", who, j);
  }
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  itemsim_drop(h);
  SimFloats scale;      // a: row_scale, b: col_scale
  SimPicks t;
  SimCsr R;
  const AlsSide& s = h->als[1];
  TRY(upload_floats(scale.a, row_scale, n));
  if (col_scale) TRY(upload_floats(scale.b, col_scale, n));
  const SimRowPlan plan = itemsim_row_plan(n);      // (both passes)
  TRY(t.alloc(n, std::max(k, ck), plan.row_floats()));

  // ---- row pass: R = the top-k of every row of Piu^alpha . Pui^alpha (. diag(col_scale)) ----
  {
    P3RowP p{};
    p.row_scale = scale.a; p.col_scale = scale.b;
    const size_t shmem = itemsim_row_args(h, 1, n, h->U, k, plan, t, &p);
    TRY(allow_lds((const void*)p3_rows_kernel, shmem));
    Scope sc(h, T_P3_ROWS, 2.0 * n * (double)s.nnz, 8.0 * n * (double)s.nnz);      // every workgroup walks the whole matrix once per slab
    GANMF_LAUNCH(p3_rows_kernel, dim3(plan.grid), dim3(KNN_THREADS), shmem, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  TRY(itemsim_compact(h, who, n, t, k, k, R));
  if (normalize) {
    Scope sc(h, T_P3_NORMALIZE, 2.0 * (double)R.nnz, 12.0 * (double)R.nnz);
    GANMF_LAUNCH(p3_normalize_kernel, dim3((unsigned)n), dim3(64), 0, h->st, (const long long*)R.indptr, R.val.get(), n);
    HIP_TRY(hipGetLastError());
  }

  // ---- column pass: the col_topk largest of every column of R; col_topk = 0: R transposed ----
  long long nnz = 0;
  if (ck > 0) {
    TRY(itemsim_columns(h, n, R, ck, plan, t));
    TRY(itemsim_compact(h, who, n, t, ck, ck, h->knn));
    nnz = h->knn.nnz;
  } else {
    HIP_TRY(hipMemsetAsync(t.cnt, 0, (size_t)n * sizeof(int), h->st));
    if (R.nnz > 0) {
      const unsigned blocks = (unsigned)std::min<long long>((R.nnz + KNN_THREADS - 1) / KNN_THREADS, 4096);
      Scope sc(h, T_P3_COLUMNS, 0.0, 8.0 * (double)R.nnz);
      GANMF_LAUNCH(p3_count_kernel, dim3(blocks), dim3(KNN_THREADS), 0, h->st, (const int*)R.indices, R.nnz, t.cnt.get());
      HIP_TRY(hipGetLastError());
    }
    std::vector<int64_t> ip;
    TRY(itemsim_indptr(h, who, t.cnt, n, n, ip));
    nnz = ip[(size_t)n];
    if (nnz != R.nnz) return fail(-2, "%s: the transposed matrix counts %lld entries of %lld", who, nnz, R.nnz);
    TRY(itemsim_alloc(ip.data(), n, h->knn));
    if (nnz > 0) {
      Scope sc(h, T_P3_COLUMNS, 0.0, 16.0 * (double)n * n);
      GANMF_LAUNCH(p3_transpose_kernel, dim3(plan.grid), dim3(KNN_THREADS), 0, h->st, (const long long*)R.indptr, (const int*)R.indices,
                   (const float*)R.val, n, (const long long*)h->knn.indptr, h->knn.indices.get(), h->knn.val.get());
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipStreamSynchronize(h->st));
  h->knn_nnz = nnz;
  *nnz_out = nnz;
  return 0;
}
