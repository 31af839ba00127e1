// abi_p3.inc -- C ABI: the graph-based item models P3alpha / RP3beta on a GANMF_MODEL_ITEMSIM handle: ganmf_p3_fit (p3_rows.hpp).  The
// result is held like ganmf_itemknn_fit's: ganmf_itemknn_get, ganmf_set_item_similarity and the scores read it unchanged.
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

// temporaries of one fit, released on every way out
struct P3FitTmp {
  float *row_scale = nullptr, *col_scale = nullptr, *row = nullptr, *val = nullptr, *r_val = nullptr;
  int *idx = nullptr, *cnt = nullptr, *r_idx = nullptr;
  long long* r_indptr = nullptr;
  ~P3FitTmp() {
    hipFree(row_scale); hipFree(col_scale); hipFree(row); hipFree(val); hipFree(r_val);
    hipFree(idx); hipFree(cnt); hipFree(r_idx); hipFree(r_indptr);
  }
};

// [n] counts from the device (enqueued behind the kernel that wrote them) to an indptr on the host
static int p3_indptr(ganmf_handle* h, const char* who, const int* cnt_dev, int n, long long most, std::vector<long long>& ip) {
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
  P3FitTmp t;
  const AlsSide& s = h->als[1];
  HIP_TRY(hipMalloc((void**)&t.row_scale, (size_t)n * sizeof(float)));
  HIP_TRY(hipMemcpy(t.row_scale, row_scale, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  if (col_scale) {
    HIP_TRY(hipMalloc((void**)&t.col_scale, (size_t)n * sizeof(float)));
    HIP_TRY(hipMemcpy(t.col_scale, col_scale, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  }
  const int row_lds = n <= KNN_ROW_LDS ? 1 : 0;
  unsigned grid = (unsigned)std::min(n, 8192);
  long long ld_row = 0;
  if (!row_lds) {      // a private row per workgroup in global memory: at most 512 of them (both passes)
    grid = (unsigned)std::min(n, 512);
    ld_row = round_up(n, LD_ALIGN);
    HIP_TRY(hipMalloc((void**)&t.row, (size_t)grid * ld_row * sizeof(float)));
  }
  const int kmax = std::max(k, ck);
  HIP_TRY(hipMalloc((void**)&t.idx, (size_t)n * kmax * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&t.val, (size_t)n * kmax * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&t.cnt, (size_t)n * sizeof(int)));

  // ---- row pass: R = the top-k of every row of Piu^alpha . Pui^alpha (. diag(col_scale)) ----
  {
    P3RowP p{};
    p.c_indptr = s.indptr; p.c_users = s.indices; p.c_val = s.conf;
    p.n_items = n; p.n_users = h->U; p.topk = k;
    p.row_scale = t.row_scale; p.col_scale = t.col_scale;
    p.slab = std::min(KNN_SLAB, round_up(h->U, 64));
    p.row_lds = row_lds; p.row_glob = t.row; p.ld_row = ld_row;
    p.out_idx = t.idx; p.out_val = t.val; p.out_cnt = t.cnt;
    const size_t shmem = ((size_t)p.slab + (row_lds ? (size_t)n : 0)) * sizeof(float);
    TRY(allow_lds((const void*)p3_rows_kernel, shmem));
    Scope sc(h, T_P3_ROWS, 2.0 * n * (double)s.nnz, 8.0 * n * (double)s.nnz);      // every workgroup walks the whole matrix once per slab
    GANMF_LAUNCH(p3_rows_kernel, dim3(grid), dim3(KNN_THREADS), shmem, h->st, p);
    HIP_TRY(hipGetLastError());
  }
  std::vector<long long> ip;
  TRY(p3_indptr(h, who, t.cnt, n, k, ip));
  const long long r_nnz = ip[(size_t)n];
  HIP_TRY(hipMalloc((void**)&t.r_indptr, ip.size() * sizeof(long long)));
  HIP_TRY(hipMalloc((void**)&t.r_idx, (size_t)std::max<long long>(r_nnz, 1) * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&t.r_val, (size_t)std::max<long long>(r_nnz, 1) * sizeof(float)));
  HIP_TRY(hipMemcpy(t.r_indptr, ip.data(), ip.size() * sizeof(long long), hipMemcpyHostToDevice));
  {
    Scope sc(h, T_KNN_PACK, 0.0, 16.0 * (double)r_nnz);
    GANMF_LAUNCH(itemknn_pack_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, h->st, (const int*)t.idx, (const float*)t.val,
                 (const int*)t.cnt, k, (const long long*)t.r_indptr, t.r_idx, t.r_val);
    HIP_TRY(hipGetLastError());
  }
  if (normalize) {
    Scope sc(h, T_P3_NORMALIZE, 2.0 * (double)r_nnz, 12.0 * (double)r_nnz);
    GANMF_LAUNCH(p3_normalize_kernel, dim3((unsigned)n), dim3(64), 0, h->st, (const long long*)t.r_indptr, t.r_val, n);
    HIP_TRY(hipGetLastError());
  }

  // ---- column pass: the col_topk largest of every column of R; col_topk = 0: R transposed ----
  if (ck > 0) {
    P3ColP p{};
    p.r_indptr = t.r_indptr; p.r_idx = t.r_idx; p.r_val = t.r_val;
    p.n_items = n; p.topk = ck;
    p.row_lds = row_lds; p.row_glob = t.row; p.ld_row = ld_row;
    p.out_idx = t.idx; p.out_val = t.val; p.out_cnt = t.cnt;
    const size_t shmem = row_lds ? (size_t)n * sizeof(float) : 0;
    TRY(allow_lds((const void*)p3_columns_kernel, shmem));
    Scope sc(h, T_P3_COLUMNS, 0.0, 16.0 * (double)n * n);
    GANMF_LAUNCH(p3_columns_kernel, dim3(grid), dim3(KNN_THREADS), shmem, h->st, p);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemsetAsync(t.cnt, 0, (size_t)n * sizeof(int), h->st));
    if (r_nnz > 0) {
      const unsigned blocks = (unsigned)std::min<long long>((r_nnz + KNN_THREADS - 1) / KNN_THREADS, 4096);
      Scope sc(h, T_P3_COLUMNS, 0.0, 8.0 * (double)r_nnz);
      GANMF_LAUNCH(p3_count_kernel, dim3(blocks), dim3(KNN_THREADS), 0, h->st, (const int*)t.r_idx, r_nnz, t.cnt);
      HIP_TRY(hipGetLastError());
    }
  }
  TRY(p3_indptr(h, who, t.cnt, n, ck > 0 ? ck : n, ip));
  const long long nnz = ip[(size_t)n];
  if (ck == 0 && nnz != r_nnz) return fail(-2, "%s: the transposed matrix counts %lld entries of %lld", who, nnz, r_nnz);
  HIP_TRY(hipMalloc((void**)&h->knn_indptr, ip.size() * sizeof(long long)));
  HIP_TRY(hipMalloc((void**)&h->knn_nbr, (size_t)std::max<long long>(nnz, 1) * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&h->knn_val, (size_t)std::max<long long>(nnz, 1) * sizeof(float)));
  HIP_TRY(hipMemcpy(h->knn_indptr, ip.data(), ip.size() * sizeof(long long), hipMemcpyHostToDevice));
  if (ck > 0) {
    Scope sc(h, T_KNN_PACK, 0.0, 16.0 * (double)nnz);
    GANMF_LAUNCH(itemknn_pack_kernel, dim3((unsigned)n), dim3(KNN_THREADS), 0, h->st, (const int*)t.idx, (const float*)t.val,
                 (const int*)t.cnt, ck, (const long long*)h->knn_indptr, h->knn_nbr, h->knn_val);
    HIP_TRY(hipGetLastError());
  } else if (nnz > 0) {
    Scope sc(h, T_P3_COLUMNS, 0.0, 16.0 * (double)n * n);
    GANMF_LAUNCH(p3_transpose_kernel, dim3(grid), dim3(KNN_THREADS), 0, h->st, (const long long*)t.r_indptr, (const int*)t.r_idx,
                 (const float*)t.r_val, n, (const long long*)h->knn_indptr, h->knn_nbr, h->knn_val);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(h->st));
  h->knn_nnz = nnz;      // set last: any failure above leaves "no matrix"
  *nnz_out = nnz;
  return 0;
}
