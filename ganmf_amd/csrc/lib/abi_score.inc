// abi_score.inc -- C ABI: scores, score filter, seen / test matrices, recommend, evaluate, scoring bench
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

// The scoring product itself: out[n, ldw] = rows[ids] . cols^T.  Many-tile shapes under the fp32-accurate default arithmetic take
// the pre-split persistent kernel (gemm_bf16p.hpp): both factors are split ONCE into their three bf16 planes (the gather of the
// scored rows rides in that pass), then one persistent launch; everything else goes through the planner (run_gemm).
static int score_product(ganmf_handle* h, const int* ids_dev, int64_t n, int transposed, int W, int ldw, bool gemm_only = false) {
  Tensor& rowsT = transposed ? h->V : h->Ue;
  Tensor& colsT = transposed ? h->Ue : h->V;
  const bool presplit = h->score_presplit && (h->tune.mode == MFMA_AUTO || h->tune.mode == MFMA_BF16X3) &&
                        h->tune.tile != 64 && bf16p_eligible((int)n, W, h->k);
  if (presplit) {
    const int mpad = round_up((int)n, BF16P_TILE), npad = round_up(W, BF16P_TILE), kp2 = round_up(h->k, BF16P_BK) / 2;
    const size_t need_a = (size_t)3 * mpad * kp2, need_b = (size_t)3 * npad * kp2;
    TRY(h->sc_pa.grow(h->st, need_a, false));
    TRY(h->sc_pb.grow(h->st, need_b, false));
    const double fl = gemm_flops((double)n, W, h->k);
    Scope s(h, T_SCORE_GEMM, fl, gemm_bytes((double)n, W, h->k));
    if (gemm_only) {      // (ganmf_bench_scores: operands prepared by the call before)
      HIP_TRY(gemm_bf16p_launch(h->st, h->sc_pa, mpad, h->sc_pb, npad, kp2, h->sc_out, ldw, (int)n, W));
      return 0;
    }
    // one split pass: the scored rows (gathered through ids) and, unless its planes are still those of the current parameters,
    // the other factor (h->param_version counts every call that can change a parameter)
    const bool b_cached = h->sc_pb_src == colsT.p && h->sc_pb_version == h->param_version && h->sc_pb_rows == W;
    const int ga = (int)std::min<long long>(4096, ((long long)mpad * kp2 + 255) / 256);
    const int gb = b_cached ? 0 : (int)std::min<long long>(4096, ((long long)npad * kp2 + 255) / 256);
    const PresplitJob ja{rowsT.p, h->ldk, ids_dev, (int)n, mpad, h->sc_pa}, jb{colsT.p, h->ldk, nullptr, W, npad, h->sc_pb};
    GANMF_LAUNCH(presplit_rows_kernel, dim3(ga + gb), dim3(256), 0, h->st, ja, jb, ga, h->k, kp2);
    HIP_TRY(hipGetLastError());
    h->sc_pb_src = colsT.p; h->sc_pb_version = h->param_version; h->sc_pb_rows = W;
    HIP_TRY(gemm_bf16p_launch(h->st, h->sc_pa, mpad, h->sc_pb, npad, kp2, h->sc_out, ldw, (int)n, W));
    return 0;
  }
  TRY(h->sc_rows.grow(h->st, (size_t)n * h->ldk, true));
  if (!gemm_only) {
    const long long total = (long long)n * (h->ldk / 4);
    GANMF_LAUNCH(gather_rows_kernel, dim3((int)std::min<long long>(2048, (total + 255) / 256)), dim3(256), 0,
                       h->st, rowsT.p.get(), h->ldk, ids_dev, (int)n, h->sc_rows.get());
    HIP_TRY(hipGetLastError());
  }
  GemmP g{};
  g.A = h->sc_rows; g.lda = h->ldk; g.B = colsT.p; g.ldb = h->ldk;
  g.C = h->sc_out; g.ldc = ldw; g.M = (int)n; g.N = W; g.K = h->k; g.epi.kind = EPI_STORE; g.c_pad_writable = 1;
  return run_gemm(h, T_SCORE_GEMM, T_RED_SCORE, g, false, false);
}

// The second score source (abi_itemknn.inc): a GANMF_MODEL_ITEMSIM handle scores through its item similarity matrix,
// out[r, i] = sum over the stored neighbours j of item i of x[u_r, j] . W[j, i].  itemsim_ready: what such a handle needs before any
// scoring entry enqueues something (0 on every other model).
static int itemsim_ready(ganmf_handle* h, const char* who, int transposed);
static int itemsim_product(ganmf_handle* h, const int* ids_dev, int64_t n, int W, int ldw);

static int scores_device(ganmf_handle* h, const int* ids_dev, int64_t n, int transposed, float** out_dev, int* width,
                         int* ld_out) {
  if (h->cfg.model == GANMF_MODEL_ITEMSIM) {      // same [n, ldw] buffer and padding as the GEMM path: everything downstream is unchanged
    TRY(itemsim_ready(h, "scores", transposed));
    const int W = h->N, ldw = round_up(W, LD_ALIGN);
    TRY(h->sc_out.grow(h->st, (size_t)n * ldw, true));
    TRY(itemsim_product(h, ids_dev, n, W, ldw));
    *out_dev = h->sc_out; *width = W; *ld_out = ldw;
    return 0;
  }
  if (h->cfg.model == GANMF_MODEL_CFGAN) {      // the third source (step_cfgan.inc): the generator's output for the rows, or rows of its transpose
    const int W = transposed ? h->U : h->N, ldw = round_up(W, LD_ALIGN);
    TRY(h->sc_out.grow(h->st, (size_t)n * ldw, true));
    TRY(cfgan_scores(h, ids_dev, n, transposed, h->sc_out, ldw));
    *out_dev = h->sc_out; *width = W; *ld_out = ldw;
    return 0;
  }
  if (h->cfg.model == GANMF_MODEL_CAAE) {      // the fourth source (step_caae.inc): sigmoid(G(profile)) of the rows
    const int W = h->N, ldw = round_up(W, LD_ALIGN);
    TRY(h->sc_out.grow(h->st, (size_t)n * ldw, true));
    TRY(caae_scores(h, ids_dev, n, transposed, h->sc_out, ldw));
    *out_dev = h->sc_out; *width = W; *ld_out = ldw;
    return 0;
  }
  Tensor& colsT = transposed ? h->Ue : h->V;   // the other factor
  const int W = colsT.rows, ldw = round_up(W, LD_ALIGN);
  TRY(h->sc_out.grow(h->st, (size_t)n * ldw, true));
  TRY(score_product(h, ids_dev, n, transposed, W, ldw));
  *out_dev = h->sc_out; *width = W; *ld_out = ldw;
  return 0;
}

// device copy of an id list in the handle's reusable buffer (scores / recommend are called once per 1000-user
// block by the evaluators: no allocation per call)
static int upload_ids(ganmf_handle* h, const int32_t* ids, int64_t n, int** out) {
  TRY(h->sc_ids.grow(h->st, (size_t)n, false));
  HIP_TRY(hipMemcpyAsync(h->sc_ids, ids, n * sizeof(int), hipMemcpyHostToDevice, h->st));
  *out = h->sc_ids;
  return 0;
}

// The filter of ganmf_set_score_filter as the two kernel arguments (item mask, indptr of the rows whose emptiness means "cold"),
// checked against the orientation in use: score width W, `limit` scored rows.
static int score_filter_args(ganmf_handle* h, const char* who, int W, int limit, const unsigned char** mask, const long long** cold) {
  *mask = nullptr; *cold = nullptr;
  if (h->item_mask_w > 0) {
    if (h->item_mask_w > W) return fail(-1, "%s: the score filter lists item %lld but the score rows have %d columns", who, (long long)h->item_mask_w - 1, W);
    *mask = h->item_mask;
  }
  if (h->mask_cold) {
    if (!h->seen.indptr || h->seen.rows != limit || h->seen.cols != W)
      return fail(-1, "%s: masking cold rows needs ganmf_set_seen_csr with a %d x %d matrix", who, limit, W);
    *cold = h->seen.indptr;
  }
  return 0;
}
static int apply_score_filter(ganmf_handle* h, const char* who, float* scores, int ld, int W, const int* ids_dev, int64_t n, int limit) {
  const unsigned char* mask; const long long* cold;
  TRY(score_filter_args(h, who, W, limit, &mask, &cold));
  if (!mask && !cold) return 0;
  GANMF_LAUNCH(score_filter_kernel, dim3((int)n), dim3(256), 0, h->st, scores, ld, W, ids_dev, mask, cold);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The keep-mask of everything that ranks while an ignore list is set: a column stays iff the score filter (if any) lists it and the
// ignore list does not.  Formed on the host from the two setters' bytes whenever either changes, so that the selection kernels keep
// their one mask pointer and ganmf_scores keeps the plain filter.  The stream is idle when the setters call this.
static int refresh_rank_mask(ganmf_handle* h) {
  if (h->ignore_w == 0) return 0;
  const size_t wmax = (size_t)std::max(h->U, h->N);
  std::vector<unsigned char> keep(wmax, 1);
  if (h->item_mask_w > 0) keep = h->filter_host;
  for (size_t i = 0; i < wmax; ++i)
    if (h->ignore_host[i]) keep[i] = 0;
  TRY(h->rank_mask.grow(h->st, wmax, false));
  HIP_TRY(hipMemcpy(h->rank_mask, keep.data(), wmax, hipMemcpyHostToDevice));
  return 0;
}
// the mask argument of the selection kernels: score_filter_args' mask, or with an ignore list the keep-mask above
static int rank_mask_arg(ganmf_handle* h, const char* who, int W, const unsigned char** mask) {
  if (h->ignore_w == 0) return 0;
  if (h->ignore_w > W) return fail(-1, "%s: the ignore list lists item %lld but the score rows have %d columns", who, (long long)h->ignore_w - 1, W);
  *mask = h->rank_mask;
  return 0;
}

int ganmf_set_score_filter(ganmf_handle* h, const int32_t* items, int64_t n_items, int mask_cold_rows) {
  if (!h) return fail(-1, "null handle");
  if (n_items < 0 || (n_items > 0 && !items)) return fail(-1, "ganmf_set_score_filter: bad item list");
  const int64_t wmax = std::max(h->U, h->N);
  int64_t top = 0;
  for (int64_t i = 0; i < n_items; ++i) {
    if (items[i] < 0 || items[i] >= wmax) return fail(-1, "ganmf_set_score_filter: item %d out of range [0,%lld)", items[i], (long long)wmax);
    top = std::max<int64_t>(top, (int64_t)items[i] + 1);
  }
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  if (n_items > 0) {
    TRY(h->item_mask.grow(h->st, (size_t)wmax, false));
    std::vector<unsigned char> m((size_t)wmax, 0);
    for (int64_t i = 0; i < n_items; ++i) m[(size_t)items[i]] = 1;
    HIP_TRY(hipMemcpy(h->item_mask, m.data(), m.size(), hipMemcpyHostToDevice));
    h->filter_host.swap(m);
  } else {
    h->filter_host.clear();
  }
  h->item_mask_w = n_items > 0 ? top : 0;
  h->mask_cold = mask_cold_rows != 0;
  return refresh_rank_mask(h);
}

int ganmf_set_items_to_ignore(ganmf_handle* h, const int32_t* items, int64_t n_items) {
  if (!h) return fail(-1, "null handle");
  if (n_items < 0 || (n_items > 0 && !items)) return fail(-1, "ganmf_set_items_to_ignore: bad item list");
  if (!items) n_items = 0;
  const int64_t wmax = std::max(h->U, h->N);
  int64_t top = 0;
  for (int64_t i = 0; i < n_items; ++i) {
    if (items[i] < 0 || items[i] >= wmax) return fail(-1, "ganmf_set_items_to_ignore: item %d out of range [0,%lld)", items[i], (long long)wmax);
    top = std::max<int64_t>(top, (int64_t)items[i] + 1);
  }
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->ignore_host.assign(n_items > 0 ? (size_t)wmax : 0, 0);
  for (int64_t i = 0; i < n_items; ++i) h->ignore_host[(size_t)items[i]] = 1;
  h->ignore_w = top;
  const int rc = refresh_rank_mask(h);
  if (rc) { h->ignore_host.clear(); h->ignore_w = 0; }     // a failed upload leaves "no ignore list"
  return rc;
}

int ganmf_scores(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, float* out) {
  if (!h || !ids || !out) return fail(-1, "ganmf_scores: null argument");
  if (n < 1 || n > (1 << 30)) return fail(-1, "ganmf_scores: n out of range");
  TRY(itemsim_ready(h, "ganmf_scores", transposed));
  const int limit = transposed ? h->N : h->U;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= limit) return fail(-1, "ganmf_scores: id %d out of range [0,%d)", ids[i], limit);
  HIP_TRY(hipSetDevice(h->dev));
  int* ids_dev = nullptr;
  TRY(upload_ids(h, ids, n, &ids_dev));
  float* od = nullptr; int W = 0, ldw = 0;
  int rc = scores_device(h, ids_dev, n, transposed, &od, &W, &ldw);
  if (rc == 0) rc = apply_score_filter(h, "ganmf_scores", od, ldw, W, ids_dev, n, limit);
  if (rc == 0) {
    hipError_t e = hipMemcpy2DAsync(out, (size_t)W * 4, od, (size_t)ldw * 4, (size_t)W * 4, n, hipMemcpyDeviceToHost, h->st);
    if (e == hipSuccess) e = hipStreamSynchronize(h->st);
    if (e != hipSuccess) rc = fail(-2, "ganmf_scores: copy back failed: %s", hipGetErrorString(e));
  }
  hipStreamSynchronize(h->st);
  return rc;
}

// The CSR arguments of a ganmf_set_*_csr entry, checked before that entry touches what it holds: monotone indptr, columns in
// [0, n_cols); require_sorted_unique: columns ascending without repeats inside a row (the test matrix, searched by bisection).
// (That entry has never refused an indptr that starts past 0 -- its rows still index the arrays it uploads -- and words its
// column message with the row; both stay.)
static int check_csr(const char* who, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, bool refuse_empty,
                     bool require_sorted_unique) {
  if (refuse_empty && (n_rows < 1 || n_cols < 1)) return fail(-1, "%s: empty matrix", who);
  const int64_t nnz = indptr[n_rows];
  if (!require_sorted_unique && (indptr[0] != 0 || nnz < 0 || (nnz > 0 && !indices))) return fail(-1, "%s: bad indptr", who);
  for (int64_t r = 0; r < n_rows; ++r)
    if (indptr[r + 1] < indptr[r]) return fail(-1, "%s: indptr not monotone at row %lld", who, (long long)r);
  for (int64_t r = 0; r < n_rows; ++r)
    for (int64_t j = indptr[r]; j < indptr[r + 1]; ++j) {
      if (indices[j] < 0 || indices[j] >= n_cols)
        return require_sorted_unique ? fail(-1, "%s: column %d out of range in row %lld", who, indices[j], (long long)r)
                                     : fail(-1, "%s: column index %d out of range", who, indices[j]);
      if (require_sorted_unique && j > indptr[r] && indices[j] <= indices[j - 1])
        return fail(-1, "%s: row %lld is not sorted / has duplicates", who, (long long)r);
    }
  return 0;
}

int ganmf_set_seen_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols) {
  if (!h || !indptr) return fail(-1, "ganmf_set_seen_csr: null argument");
  TRY(check_csr("ganmf_set_seen_csr", indptr, indices, n_rows, n_cols, false, false));
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  return h->seen.upload(indptr, indices, n_rows, n_cols);
}

// a launch with `shmem` bytes of dynamic LDS: past the 48 KiB every kernel may ask for, the kernel has to be told first
static int allow_lds(const void* kernel, size_t shmem) {
  if (shmem > 48 * 1024) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  return 0;
}

// The ranking front of ganmf_recommend[_candidates] and of every ganmf_evaluate*: the top-`cutoff` of the rows `ids`, left on the
// device in h->topk_items / h->topk_vals ([n, cutoff]); *ids_dev_out = the uploaded ids.  cand = false: full width, scores -> seen
// mask -> selection (scores_device + mask_topk_kernel).  cand = true: each row among its own candidates (cand_topk.hpp), no score
// row formed.  rmse != nullptr (the 13-sum evaluations): the selection kernel also writes each row's RMSE over its test items.
// Every check runs before anything is enqueued.
static int rank_device(ganmf_handle* h, const char* who, bool cand, const int32_t* ids, int64_t n, int transposed, int32_t cutoff,
                       int remove_seen, int** ids_dev_out, const RmseP* rmse) {
  if (n < 1 || n > (1 << 30)) return fail(-1, "%s: n out of range", who);
  if (cand) TRY(needs_tensors(h, who));      // (candidate scoring gathers factor rows)
  if (cand) TRY(not_cfgan(h, who));
  TRY(itemsim_ready(h, who, transposed));
  const int limit = transposed ? h->N : h->U, W = transposed ? h->U : h->N;
  if (cand && !h->cand.indptr) return fail(-1, "%s: no candidate matrix (ganmf_set_candidates_csr)", who);
  if (cand && (h->cand.rows != limit || h->cand.cols != W))
    return fail(-1, "%s: the candidate matrix is %lld x %lld, transposed = %d needs %d x %d", who, (long long)h->cand.rows,
                (long long)h->cand.cols, transposed, limit, W);
  if (cutoff < 1 || cutoff > W || cutoff > GANMF_RECOMMEND_MAX_CUTOFF)
    return fail(-1, "%s: cutoff %d out of range [1,%d]", who, cutoff, std::min(W, GANMF_RECOMMEND_MAX_CUTOFF));
  long long longest = 0;      // (candidate lists of the rows asked for)
  for (int64_t i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= limit) return fail(-1, "%s: id %d out of range [0,%d)", who, ids[i], limit);
    if (!cand) continue;
    const long long len = h->cand_indptr_host[(size_t)ids[i] + 1] - h->cand_indptr_host[(size_t)ids[i]];
    if (len > CAND_MAX_PER_ROW)
      return fail(-1, "%s: row %d has %lld candidates, at most %d (GANMF_CANDIDATES_MAX_PER_ROW)", who, ids[i], len, CAND_MAX_PER_ROW);
    longest = std::max(longest, len);
  }
  if (remove_seen && (!h->seen.indptr || h->seen.rows != limit || h->seen.cols != W))
    return fail(-1, "%s: remove_seen needs ganmf_set_seen_csr with a %d x %d matrix", who, limit, W);
  const unsigned char* fmask; const long long* fcold;
  TRY(score_filter_args(h, who, W, limit, &fmask, &fcold));
  TRY(rank_mask_arg(h, who, W, &fmask));
  const int cand_cap = round_up((int)std::max<long long>(longest, 1), 64);
  const size_t cand_shmem = ((size_t)2 * cand_cap + (h->ldk > CAND_REG_LD ? (size_t)h->ldk : 0)) * sizeof(float);
  if (cand && cand_shmem > 144 * 1024)
    return fail(-1, "%s: %d factors beside %lld candidates do not fit one workgroup's LDS", who, h->k, longest);
  HIP_TRY(hipSetDevice(h->dev));
  int* ids_dev = nullptr;
  TRY(upload_ids(h, ids, n, &ids_dev));
  {   // the two top-k buffers: the count is published (topk_vals.cap) once both hold n * cutoff
    const size_t need = (size_t)n * cutoff;
    if (need > h->topk_vals.cap) h->topk_vals.reset();      // (topk_vals grows last: its cap is what both hold)
    TRY(h->topk_items.grow(h->st, need, false));
    TRY(h->topk_vals.grow(h->st, need, false));
  }
  const long long* seen_indptr = remove_seen ? h->seen.indptr : nullptr;
  if (cand) {
    Tensor& rowsT = transposed ? h->V : h->Ue;
    Tensor& colsT = transposed ? h->Ue : h->V;
    CandP p{};
    p.cap = cand_cap;
    p.rows = rowsT.p; p.cols = colsT.p; p.ld = h->ldk; p.k = h->k; p.ids = ids_dev;
    p.c_indptr = h->cand.indptr; p.c_indices = h->cand.indices;
    p.seen_indptr = seen_indptr; p.seen_indices = h->seen.indices;
    p.item_mask = fmask; p.cold_indptr = fcold; p.cutoff = cutoff;
    p.out_items = h->topk_items; p.out_vals = h->topk_vals;
    TRY(allow_lds(rmse ? reinterpret_cast<const void*>(cand_topk_rmse_kernel) : reinterpret_cast<const void*>(cand_topk_kernel), cand_shmem));
    if (rmse) GANMF_LAUNCH(cand_topk_rmse_kernel, dim3((int)n), dim3(256), cand_shmem, h->st, p, *rmse);
    else GANMF_LAUNCH(cand_topk_kernel, dim3((int)n), dim3(256), cand_shmem, h->st, p);
  } else {
    float* od = nullptr; int Wd = 0, ldw = 0;
    TRY(scores_device(h, ids_dev, n, transposed, &od, &Wd, &ldw));
    const int lds_cap = 32768;   // floats: 128 KiB of the CU's 160 KiB
    const size_t shmem = Wd <= lds_cap ? (size_t)Wd * sizeof(float) : 0;
    TRY(allow_lds(rmse ? reinterpret_cast<const void*>(mask_topk_rmse_kernel) : reinterpret_cast<const void*>(mask_topk_kernel), shmem));
    if (rmse)
      GANMF_LAUNCH(mask_topk_rmse_kernel, dim3((int)n), dim3(256), shmem, h->st, od, ldw, Wd, ids_dev, seen_indptr, h->seen.indices.get(),
                   (int)cutoff, lds_cap, h->topk_items.get(), h->topk_vals.get(), fmask, fcold, *rmse);
    else
      GANMF_LAUNCH(mask_topk_kernel, dim3((int)n), dim3(256), shmem, h->st, od, ldw, Wd, ids_dev, seen_indptr, h->seen.indices.get(),
                   (int)cutoff, lds_cap, h->topk_items.get(), h->topk_vals.get(), fmask, fcold);
  }
  HIP_TRY(hipGetLastError());
  if (ids_dev_out) *ids_dev_out = ids_dev;
  return 0;
}

// the [n, cutoff] lists rank_device left on the device, to the caller's arrays
static int copy_topk(ganmf_handle* h, const char* who, int64_t n, int32_t cutoff, int32_t* out_items, float* out_scores) {
  const size_t need = (size_t)n * cutoff;
  hipError_t e = hipMemcpyAsync(out_items, h->topk_items, need * sizeof(int), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess && out_scores) e = hipMemcpyAsync(out_scores, h->topk_vals, need * sizeof(float), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  return e == hipSuccess ? 0 : fail(-2, "%s: %s", who, hipGetErrorString(e));
}

int ganmf_recommend(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int32_t cutoff, int remove_seen,
                    int32_t* out_items, float* out_scores) {
  if (!h || !ids || !out_items) return fail(-1, "ganmf_recommend: null argument");
  int rc = rank_device(h, "ganmf_recommend", false, ids, n, transposed, cutoff, remove_seen, nullptr, nullptr);
  if (rc == 0) rc = copy_topk(h, "ganmf_recommend", n, cutoff, out_items, out_scores);
  hipStreamSynchronize(h->st);
  return rc;
}

int ganmf_set_candidates_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols) {
  if (!h) return fail(-1, "null handle");
  if (indptr) TRY(check_csr("ganmf_set_candidates_csr", indptr, indices, n_rows, n_cols, true, false));
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->cand.drop();
  h->cand_indptr_host.clear();
  if (!indptr) return 0;
  // canonical rows (columns ascending, a repeated column kept once), as ganmf_set_urm_csr makes the training matrix canonical
  std::vector<long long> ip((size_t)n_rows + 1, 0);
  std::vector<int> ix;
  ix.reserve((size_t)indptr[n_rows]);
  for (int64_t r = 0; r < n_rows; ++r) {
    const size_t at = ix.size();
    ix.insert(ix.end(), indices + indptr[r], indices + indptr[r + 1]);
    std::sort(ix.begin() + at, ix.end());
    ix.erase(std::unique(ix.begin() + at, ix.end()), ix.end());
    ip[(size_t)r + 1] = (long long)ix.size();
  }
  TRY(h->cand.upload(ip.data(), ix.data(), n_rows, n_cols));      // a failed upload leaves "no candidate matrix"
  h->cand_indptr_host.swap(ip);
  return 0;
}

int ganmf_recommend_candidates(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int32_t cutoff, int remove_seen,
                               int32_t* out_items, float* out_scores) {
  if (!h || !ids || !out_items) return fail(-1, "ganmf_recommend_candidates: null argument");
  int rc = rank_device(h, "ganmf_recommend_candidates", true, ids, n, transposed, cutoff, remove_seen, nullptr, nullptr);
  if (rc == 0) rc = copy_topk(h, "ganmf_recommend_candidates", n, cutoff, out_items, out_scores);
  hipStreamSynchronize(h->st);
  return rc;
}

int ganmf_set_test_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const double* gains, int64_t n_rows,
                       int64_t n_cols) {
  if (!h || !indptr || (!indices && indptr[n_rows] > 0) || (!gains && indptr[n_rows] > 0)) return fail(-1, "ganmf_set_test_csr: null argument");
  TRY(check_csr("ganmf_set_test_csr", indptr, indices, n_rows, n_cols, true, true));
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->test_gain.reset();
  h->test_rating.reset(); h->test_rating_ok = false;      // the ratings belong to the matrix they were set for
  TRY(h->test.upload(indptr, indices, n_rows, n_cols));
  return h->test.upload_values(h->test_gain, gains);
}

int ganmf_set_test_ratings(ganmf_handle* h, const float* ratings, int64_t nnz) {
  if (!h || (nnz > 0 && !ratings)) return fail(-1, "ganmf_set_test_ratings: null argument");
  if (!h->test.indptr) return fail(-1, "ganmf_set_test_ratings: needs ganmf_set_test_csr first");
  if (nnz != h->test.nnz) return fail(-1, "ganmf_set_test_ratings: %lld ratings for a test matrix of %lld entries", (long long)nnz, (long long)h->test.nnz);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->test_rating.reset(); h->test_rating_ok = false;
  TRY(h->test_rating.alloc((size_t)std::max<int64_t>(nnz, 1), false));
  if (nnz > 0) HIP_TRY(hipMemcpy(h->test_rating, ratings, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
  h->test_rating_ok = true;
  return 0;
}

int ganmf_set_eval_item_weights(ganmf_handle* h, const double* novelty, const double* popularity, int64_t width) {
  if (!h || !novelty || !popularity) return fail(-1, "ganmf_set_eval_item_weights: null argument");
  if (width < 1 || width > std::max(h->U, h->N)) return fail(-1, "ganmf_set_eval_item_weights: width %lld out of range", (long long)width);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->eval_w_width = 0;
  TRY(h->eval_w.alloc((size_t)2 * width, false));
  HIP_TRY(hipMemcpy(h->eval_w, novelty, (size_t)width * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->eval_w + width, popularity, (size_t)width * sizeof(double), hipMemcpyHostToDevice));
  h->eval_w_width = width;
  return 0;
}

// What every ganmf_evaluate* shares.  eval_prepare makes the argument checks, ranks the rows (rank_device, to the largest cut-off K)
// and stages the metric kernels' inputs in h->eval_buf, laid out  disc [K] | ideal_cum [n, K] | tail [tail]  (the tail is the
// caller's: block partials, or per-user values and group sums); `p` is ready but for p.partials.
struct EvalCall { int K, W; double *d_disc, *d_ideal, *d_tail; EvalP p; };

// full: the 13-sum form, which also needs the ratings and the item weights, and whose ranking writes every row's RMSE to h->eval_rmse
static int eval_prepare(ganmf_handle* h, const char* who, bool cand, bool full, const int32_t* ids, int64_t n, int transposed,
                        int remove_seen, const int32_t* cutoffs, int32_t n_cutoffs, const double* disc, const double* ideal_cum,
                        size_t tail, EvalCall* c) {
  if (!h || !ids || !cutoffs || !disc || !ideal_cum) return fail(-1, "%s: null argument", who);
  if (n_cutoffs < 1 || n_cutoffs > GANMF_EVAL_MAX_CUTOFFS) return fail(-1, "%s: 1..%d cut-offs per call", who, GANMF_EVAL_MAX_CUTOFFS);
  if (n < 1 || n > (1 << 30)) return fail(-1, "%s: n out of range", who);
  const int limit = transposed ? h->N : h->U, W = transposed ? h->U : h->N;
  if (!h->test.indptr || h->test.rows != limit || h->test.cols != W)
    return fail(-1, "%s: needs ganmf_set_test_csr with a %d x %d matrix", who, limit, W);
  if (full && !h->test_rating_ok) return fail(-1, "%s: needs ganmf_set_test_ratings for the current test matrix", who);
  if (full && h->eval_w_width != W) return fail(-1, "%s: needs ganmf_set_eval_item_weights of width %d", who, W);
  int K = 0;
  for (int i = 0; i < n_cutoffs; ++i) {
    if (cutoffs[i] < 1) return fail(-1, "%s: cut-off %d", who, cutoffs[i]);
    K = std::max(K, (int)cutoffs[i]);
  }
  HIP_TRY(hipSetDevice(h->dev));
  if (full) {
    TRY(h->eval_rmse.grow(h->st, (size_t)n, false));
    TRY(h->eval_counts.grow(h->st, (size_t)n_cutoffs * W, false));
  }
  const RmseP rp{h->test.indptr, h->test.indices, h->test_rating, h->eval_rmse};
  int* ids_dev = nullptr;
  TRY(rank_device(h, who, cand, ids, n, transposed, K, remove_seen, &ids_dev, full ? &rp : nullptr));
  TRY(h->eval_buf.grow(h->st, (size_t)K + (size_t)n * K + tail, false));
  c->K = K; c->W = W;
  c->d_disc = h->eval_buf;
  c->d_ideal = c->d_disc + K;
  c->d_tail = c->d_ideal + (size_t)n * K;
  HIP_TRY(hipMemcpyAsync(c->d_disc, disc, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->st));
  HIP_TRY(hipMemcpyAsync(c->d_ideal, ideal_cum, (size_t)n * K * sizeof(double), hipMemcpyHostToDevice, h->st));
  EvalP& p = c->p;
  p = EvalP{};
  p.items = h->topk_items; p.K = K; p.n = (int)n; p.ids = ids_dev;
  p.t_indptr = h->test.indptr; p.t_indices = h->test.indices; p.t_gain = h->test_gain;
  p.disc = c->d_disc; p.ideal_cum = c->d_ideal; p.ncut = n_cutoffs; p.partials = nullptr;
  for (int i = 0; i < n_cutoffs; ++i) p.cutoffs[i] = cutoffs[i];
  return 0;
}

// sums[ncol] of the [grid, ncol] block partials: blocks ascending, one running sum per column (reproducible)
static void sum_block_partials(const std::vector<double>& part, int grid, int ncol, double* sums) {
  for (int i = 0; i < ncol; ++i) sums[i] = 0.0;
  for (int b = 0; b < grid; ++b)
    for (int i = 0; i < ncol; ++i) sums[i] += part[(size_t)b * ncol + i];
}

// ganmf_evaluate, ganmf_evaluate_full (cand = false: full-width ranking) and ganmf_evaluate_candidates (cand = true: each row's own
// candidate list).  counts == nullptr: the nine sums of EVAL_METRICS per cut-off; given: the 13 of EVAL_FULL_METRICS, and the lists'
// per-item counts added into `counts`.
static int evaluate_device(ganmf_handle* h, const char* who, bool cand, const int32_t* ids, int64_t n, int transposed, int remove_seen,
                           const int32_t* cutoffs, int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums,
                           int64_t* counts) {
  if (!sums) return fail(-1, "%s: null argument", who);
  const bool full = counts != nullptr;
  const int grid = (int)((n + 255) / 256), ncol = n_cutoffs * (full ? EVAL_FULL_METRICS : EVAL_METRICS);
  const size_t n_part = (size_t)grid * ncol;
  EvalCall c;
  TRY(eval_prepare(h, who, cand, full, ids, n, transposed, remove_seen, cutoffs, n_cutoffs, disc, ideal_cum, n_part, &c));
  c.p.partials = c.d_tail;
  const size_t n_counts = full ? (size_t)n_cutoffs * c.W : 0;
  if (full) {
    HIP_TRY(hipMemsetAsync(h->eval_counts, 0, n_counts * sizeof(unsigned), h->st));
    EvalFullP f{};
    f.rmse = h->eval_rmse; f.w_nov = h->eval_w; f.w_pop = h->eval_w + c.W; f.counts = h->eval_counts; f.W = c.W;
    for (int i = 0; i < n_cutoffs; ++i) f.order[i] = i;
    std::stable_sort(f.order, f.order + n_cutoffs, [&](int a, int b) { return cutoffs[a] < cutoffs[b]; });
    const size_t hist_bytes = n_counts * sizeof(unsigned);
    f.lds_counts = hist_bytes <= EVAL_COUNTS_LDS_BYTES ? 1 : 0;
    const size_t shmem = f.lds_counts ? hist_bytes : 0;
    TRY(allow_lds(reinterpret_cast<const void*>(eval_topk_full_kernel), shmem));
    GANMF_LAUNCH(eval_topk_full_kernel, dim3(grid), dim3(256), shmem, h->st, c.p, f);
  } else {
    GANMF_LAUNCH(eval_topk_kernel, dim3(grid), dim3(256), 0, h->st, c.p);
  }
  HIP_TRY(hipGetLastError());
  std::vector<double> part(n_part);
  std::vector<unsigned> cnt(n_counts);
  HIP_TRY(hipMemcpyAsync(part.data(), c.d_tail, n_part * sizeof(double), hipMemcpyDeviceToHost, h->st));
  if (full) HIP_TRY(hipMemcpyAsync(cnt.data(), h->eval_counts, n_counts * sizeof(unsigned), hipMemcpyDeviceToHost, h->st));
  HIP_TRY(hipStreamSynchronize(h->st));
  sum_block_partials(part, grid, ncol, sums);
  for (size_t i = 0; i < n_counts; ++i) counts[i] += (int64_t)cnt[i];
  return 0;
}

int ganmf_evaluate(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, const int32_t* cutoffs,
                   int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums) {
  return evaluate_device(h, "ganmf_evaluate", false, ids, n, transposed, remove_seen, cutoffs, n_cutoffs, disc, ideal_cum, sums, nullptr);
}

int ganmf_evaluate_full(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, const int32_t* cutoffs,
                        int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums, int64_t* counts) {
  if (!counts) return fail(-1, "ganmf_evaluate_full: null argument");
  return evaluate_device(h, "ganmf_evaluate_full", false, ids, n, transposed, remove_seen, cutoffs, n_cutoffs, disc, ideal_cum, sums, counts);
}

int ganmf_evaluate_candidates(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, const int32_t* cutoffs,
                              int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums, int64_t* counts) {
  return evaluate_device(h, "ganmf_evaluate_candidates", true, ids, n, transposed, remove_seen, cutoffs, n_cutoffs, disc, ideal_cum, sums,
                         counts);
}

// ganmf_evaluate_groups: the ranking of ganmf_evaluate (candidates = 0) or ganmf_evaluate_candidates (candidates = 1), then every user's
// own metric values (eval_topk_users_kernel) instead of their sum, and the sums of those values per group of users in a fixed order
// (eval_group_sum_kernel).  Every argument check runs before anything is enqueued.
static_assert(EVAL_MAX_GROUPS == GANMF_EVAL_MAX_GROUPS, "group limit of the kernels and of the header");
int ganmf_evaluate_groups(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, int candidates,
                          const int32_t* cutoffs, int32_t n_cutoffs, const double* disc, const double* ideal_cum,
                          const int32_t* group_of, int32_t n_groups, double* group_sums, int64_t* group_size, double* per_user) {
  const char* who = "ganmf_evaluate_groups";
  if (n_groups < 0 || n_groups > GANMF_EVAL_MAX_GROUPS) return fail(-1, "%s: %d groups, 0..%d per call", who, n_groups, GANMF_EVAL_MAX_GROUPS);
  if (n_groups == 0 && !per_user) return fail(-1, "%s: neither groups nor per_user asked for", who);
  if (n_groups > 0 && (!group_of || !group_sums || !group_size)) return fail(-1, "%s: null group argument", who);
  // members of every group: positions of `ids`, ascending inside a group (counting sort) -- the order the sums are formed in
  const int G = n_groups;
  std::vector<int> begin((size_t)G + 1, 0), members;
  if (G > 0) {
    for (int64_t i = 0; i < n; ++i) {
      if (group_of[i] < -1 || group_of[i] >= G)
        return fail(-1, "%s: group_of[%lld] = %d out of range [-1,%d)", who, (long long)i, group_of[i], G);
      if (group_of[i] >= 0) ++begin[(size_t)group_of[i] + 1];
    }
    for (int g = 0; g < G; ++g) begin[(size_t)g + 1] += begin[(size_t)g];
    members.resize((size_t)std::max(begin[(size_t)G], 1));
    std::vector<int> at(begin.begin(), begin.end() - 1);
    for (int64_t i = 0; i < n; ++i)
      if (group_of[i] >= 0) members[(size_t)at[(size_t)group_of[i]]++] = (int)i;
  }
  const int ncol = n_cutoffs * EVAL_METRICS;
  const size_t n_user = (size_t)n * ncol, n_sum = (size_t)G * ncol;
  EvalCall c;
  TRY(eval_prepare(h, who, candidates != 0, false, ids, n, transposed, remove_seen, cutoffs, n_cutoffs, disc, ideal_cum, n_user + n_sum, &c));
  TRY(h->eval_grp.grow(h->st, G > 0 ? members.size() + begin.size() : 0, false));
  double* d_user = c.d_tail;
  double* d_sum = d_user + n_user;
  {
    Scope s(h, T_EVAL_GROUPS, 0.0, 4.0 * n * c.K + 8.0 * n * c.K + 8.0 * n_user);
    GANMF_LAUNCH(eval_topk_users_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, c.p, d_user);
    HIP_TRY(hipGetLastError());
  }
  hipError_t e = hipSuccess;
  if (G > 0) {
    int* d_members = h->eval_grp;
    int* d_begin = d_members + members.size();
    e = hipMemcpyAsync(d_members, members.data(), members.size() * sizeof(int), hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_begin, begin.data(), begin.size() * sizeof(int), hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) {
      Scope s(h, T_EVAL_GROUPS, (double)begin[(size_t)G] * ncol, 12.0 * begin[(size_t)G] * ncol + 8.0 * n_sum);
      GANMF_LAUNCH(eval_group_sum_kernel, dim3((unsigned)G, (unsigned)ncol), dim3(256), 0, h->st, d_user, ncol, d_members, d_begin, d_sum);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(group_sums, d_sum, n_sum * sizeof(double), hipMemcpyDeviceToHost, h->st);
  }
  if (e == hipSuccess && per_user) e = hipMemcpyAsync(per_user, d_user, n_user * sizeof(double), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  if (e != hipSuccess) { hipStreamSynchronize(h->st); return fail(-2, "%s: %s", who, hipGetErrorString(e)); }   // (members / begin are locals)
  for (int g = 0; g < G; ++g) group_size[g] = (int64_t)(begin[(size_t)g + 1] - begin[(size_t)g]);
  return 0;
}

// ---- ganmf_set_item_diversity / ganmf_evaluate_diversity (list_diversity.hpp) ----------------------------------------------------
int ganmf_set_item_diversity(ganmf_handle* h, const float* matrix, int64_t width) {
  const char* who = "ganmf_set_item_diversity";
  if (!h) return fail(-1, "null handle");
  if (matrix && (width < 1 || width > std::max(h->U, h->N))) return fail(-1, "%s: width %lld out of range", who, (long long)width);
  HIP_TRY(hipSetDevice(h->dev));
  HIP_TRY(hipStreamSynchronize(h->st));
  h->div_mat.reset(); h->div_w = 0;
  if (!matrix) return 0;
  const size_t bytes = (size_t)width * (size_t)width * sizeof(float);
  size_t free_b = 0, total_b = 0;     // never more than a quarter of the free device memory (the rule of ganmf_score_similarity)
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 4)
    return fail(-1, "%s: out of memory budget: a %lld x %lld matrix needs %.1f MB, over a quarter of the %.1f MB free", who,
                (long long)width, (long long)width, bytes / 1048576.0, free_b / 1048576.0);
  TRY(h->div_mat.alloc((size_t)width * (size_t)width, false));
  HIP_TRY(hipMemcpy(h->div_mat, matrix, bytes, hipMemcpyHostToDevice));
  h->div_w = width;                   // set last: a failed upload leaves "no matrix"
  return 0;
}

int ganmf_evaluate_diversity(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, int candidates,
                             const int32_t* cutoffs, int32_t n_cutoffs, double* sums, double* per_user) {
  const char* who = "ganmf_evaluate_diversity";
  if (!h || !ids || !cutoffs || !sums) return fail(-1, "%s: null argument", who);
  if (n_cutoffs < 1 || n_cutoffs > GANMF_EVAL_MAX_CUTOFFS) return fail(-1, "%s: 1..%d cut-offs per call", who, GANMF_EVAL_MAX_CUTOFFS);
  const int W = transposed ? h->U : h->N;
  if (!h->div_mat) return fail(-1, "%s: no diversity matrix (ganmf_set_item_diversity)", who);
  if (h->div_w != W) return fail(-1, "%s: the diversity matrix has width %lld, the score rows have %d columns", who, (long long)h->div_w, W);
  ListDivP p{};
  int K = 0;
  for (int i = 0; i < n_cutoffs; ++i) {
    if (cutoffs[i] < 1) return fail(-1, "%s: cut-off %d", who, cutoffs[i]);
    K = std::max(K, (int)cutoffs[i]);
    p.cutoffs[i] = cutoffs[i]; p.order[i] = i;
  }
  static_assert(LIST_DIV_MAX_K == GANMF_RECOMMEND_MAX_CUTOFF, "the kernel's LDS list holds the longest list rank_device takes");
  std::stable_sort(p.order, p.order + n_cutoffs, [&](int a, int b) { return cutoffs[a] < cutoffs[b]; });
  TRY(rank_device(h, who, candidates != 0, ids, n, transposed, K, remove_seen, nullptr, nullptr));     // (refuses K over the limit)
  const int grid = (int)((n + 255) / 256);
  const size_t n_user = (size_t)n * n_cutoffs, n_part = (size_t)grid * n_cutoffs;
  TRY(h->eval_buf.grow(h->st, n_user + n_part, false));
  double* d_user = h->eval_buf;
  double* d_part = d_user + n_user;
  p.items = h->topk_items; p.K = K; p.D = h->div_mat; p.W = W; p.ncut = n_cutoffs; p.out = d_user;
  // (no profile class, like the selection kernels: it is not timed per class)
  GANMF_LAUNCH(list_diversity_kernel, dim3((unsigned)n), dim3(256), 0, h->st, p);
  HIP_TRY(hipGetLastError());
  GANMF_LAUNCH(column_block_sum_kernel, dim3((unsigned)grid, (unsigned)n_cutoffs), dim3(256), 0, h->st, d_user, (int)n, (int)n_cutoffs, d_part);
  HIP_TRY(hipGetLastError());
  std::vector<double> part(n_part);
  hipError_t e = hipMemcpyAsync(part.data(), d_part, n_part * sizeof(double), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess && per_user) e = hipMemcpyAsync(per_user, d_user, n_user * sizeof(double), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  if (e != hipSuccess) { hipStreamSynchronize(h->st); return fail(-2, "%s: %s", who, hipGetErrorString(e)); }
  sum_block_partials(part, grid, n_cutoffs, sums);
  return 0;
}

int ganmf_bench_scores(ganmf_handle* h, int64_t n, int transposed, int32_t iters, float* ms_per_launch) {
  if (!h || iters < 1) return fail(-1, "ganmf_bench_scores: bad argument");
  TRY(needs_tensors(h, "ganmf_bench_scores"));
  TRY(not_cfgan(h, "ganmf_bench_scores"));
  const int limit = transposed ? h->N : h->U;
  if (n < 1 || n > limit) return fail(-1, "ganmf_bench_scores: n out of range");
  HIP_TRY(hipSetDevice(h->dev));
  std::vector<int> ids(n);
  for (int64_t i = 0; i < n; ++i) ids[i] = (int)i;
  int* ids_dev = nullptr;
  TRY(upload_ids(h, ids.data(), n, &ids_dev));
  HIP_TRY(hipStreamSynchronize(h->st));      // `ids` is a local: the copy must be done before it goes away
  float* od; int W, ldw;
  int rc = scores_device(h, ids_dev, n, transposed, &od, &W, &ldw);  // warm-up + allocation
  if (rc) return rc;
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  const bool was = h->prof;
  h->prof = false;
  // Default: the GEMM launch alone on prepared operands (what this entry has always timed).  GANMF_BENCH_SCORES_PRODUCT=1: the whole
  // product per iteration -- the gather of the scored rows, or on the pre-split kernel BOTH split passes (as the first scoring
  // call after a training epoch pays them), + the GEMM.
  const bool whole = tune_env_int("score_product", 0) != 0;
  score_product(h, ids_dev, n, transposed, W, ldw);
  hipEventRecord(a, h->st);
  for (int i = 0; i < iters; ++i) {
    if (whole) h->sc_pb_version = -1;
    score_product(h, ids_dev, n, transposed, W, ldw, !whole);
  }
  h->prof = was;
  hipEventRecord(b, h->st);
  hipError_t e = hipEventSynchronize(b);
  float ms = 0.f;
  hipEventElapsedTime(&ms, a, b);
  hipEventDestroy(a); hipEventDestroy(b);
  if (e != hipSuccess) return fail(-2, "ganmf_bench_scores: %s", hipGetErrorString(e));
  if (ms_per_launch) *ms_per_launch = ms / iters;
  return 0;
}

// ---- ganmf_score_similarity (gram_stats.hpp) ---------------------------------------------------------------------------------
constexpr int64_t SIM_MAX_ROWS = 1 << 22;      // 32 768 tile rows: the tiles of the upper triangle still fit a 1-D grid

int ganmf_score_similarity(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int32_t pool, double sums[4], float* pooled,
                           float* matrix) {
  const char* who = "ganmf_score_similarity";
  if (!h || !ids || !sums) return fail(-1, "%s: null argument", who);
  TRY(needs_tensors(h, who));
  if (n < 1 || n > SIM_MAX_ROWS) return fail(-1, "%s: n out of range [1,%lld]", who, (long long)SIM_MAX_ROWS);
  const int limit = transposed ? h->N : h->U;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= limit) return fail(-1, "%s: id %d out of range [0,%d)", who, ids[i], limit);
  if (pooled && (pool < 1 || pool > std::min<int64_t>(n, 1024)))
    return fail(-1, "%s: pool %d out of range [1,%lld]", who, pool, (long long)std::min<int64_t>(n, 1024));
  const int W = transposed ? h->U : h->N, ldw = round_up(W, LD_ALIGN), ldn = round_up((int)n, LD_ALIGN);
  const bool want_mat = pooled != nullptr || matrix != nullptr;
  const int nt = ((int)n + GRAM_TILE - 1) / GRAM_TILE;
  const long long tiles = gram_row_start(nt, nt);
  const size_t need_out = (size_t)n * ldw, need_mat = want_mat ? (size_t)n * ldn : 0, need_pool = pooled ? (size_t)pool * pool : 0;
  HIP_TRY(hipSetDevice(h->dev));
  {   // never more than a quarter of the free device memory for what this call adds to the handle (the rule of the pass buffers)
    size_t grow = 0, free_b = 0, total_b = 0;
    if (need_out > h->sc_out.cap) grow += (need_out - h->sc_out.cap) * sizeof(float);
    if (need_mat > h->sim_mat.cap) grow += (need_mat - h->sim_mat.cap) * sizeof(float);
    if (need_pool > h->sim_pool.cap) grow += (need_pool - h->sim_pool.cap) * sizeof(float);
    if ((size_t)2 * tiles > h->sim_part.cap) grow += ((size_t)2 * tiles - h->sim_part.cap) * sizeof(double);
    if (grow > 0 && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || grow > free_b / 4))
      return fail(-1, "%s: %lld rows%s need %.1f MB more device memory, over a quarter of the %.1f MB free", who, (long long)n,
                  want_mat ? " with their similarity matrix" : "", grow / 1048576.0, free_b / 1048576.0);
  }
  int* ids_dev = nullptr;
  TRY(upload_ids(h, ids, n, &ids_dev));
  TRY(h->sim_mat.grow(h->st, need_mat, false));
  TRY(h->sim_pool.grow(h->st, need_pool, false));
  TRY(h->sim_part.grow(h->st, (size_t)2 * tiles, false));
  TRY(h->sim_zero.grow(h->st, (size_t)n, false));
  float* sd = nullptr; int Wd = 0, ldd = 0;
  int rc = scores_device(h, ids_dev, n, transposed, &sd, &Wd, &ldd);      // unfiltered: a -inf has no cosine
  if (rc) { hipStreamSynchronize(h->st); return rc; }
  {
    Scope s(h, T_SIM_AUX, 3.0 * n * W, 8.0 * n * ldw);
    GANMF_LAUNCH(sim_normalize_kernel, dim3((int)n), dim3(256), 0, h->st, sd, ldd, Wd, h->sim_zero.get());
    HIP_TRY(hipGetLastError());
  }
  {
    GemmP g{};
    g.A = sd; g.B = sd; g.lda = ldd; g.ldb = ldd;
    g.C = want_mat ? h->sim_mat : nullptr; g.ldc = ldn;
    g.M = (int)n; g.N = (int)n; g.K = Wd;
    g.zero_page = h->zero_page;
    g.nsplit = 1; g.k_per_split = round_up(Wd, GEMM_K_ALIGN); g.nbatch = 1;
    g.tiles_m = nt; g.tiles_n = nt;
    g.epi.kind = EPI_GRAM_STATS; g.epi.gram_partials = h->sim_part;
    // (flops: the tiles that run, 2 * 128 * 128 * K each -- what the launch executes, against the MFMA roof)
    Scope s(h, T_SIM_GRAM, 2.0 * tiles * GRAM_TILE * GRAM_TILE * Wd, 4.0 * n * ldw + (want_mat ? 4.0 * n * n : 0.0));
    if (h->gram_arith == 1) GANMF_LAUNCH(gram_bf16x3_kernel, dim3((unsigned)tiles), dim3(256), 0, h->st, g);
    else GANMF_LAUNCH(gram_f32_kernel, dim3((unsigned)tiles), dim3(256), 0, h->st, g);
    HIP_TRY(hipGetLastError());
  }
  std::vector<double> part((size_t)2 * tiles);
  std::vector<int> zr((size_t)n);
  hipError_t e = hipMemcpyAsync(part.data(), h->sim_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess) e = hipMemcpyAsync(zr.data(), h->sim_zero, zr.size() * sizeof(int), hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess && pooled) {
    {
      Scope s(h, T_SIM_AUX, (double)n * n, 4.0 * n * n);
      GANMF_LAUNCH(sim_pool_kernel, dim3((unsigned)(pool * pool)), dim3(256), 0, h->st, h->sim_mat.get(), ldn, (int)n, (int)pool, h->sim_pool.get());
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(pooled, h->sim_pool, need_pool * sizeof(float), hipMemcpyDeviceToHost, h->st);
  }
  if (e == hipSuccess && matrix)
    e = hipMemcpy2DAsync(matrix, (size_t)n * 4, h->sim_mat, (size_t)ldn * 4, (size_t)n * 4, n, hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  if (e != hipSuccess) { hipStreamSynchronize(h->st); return fail(-2, "%s: %s", who, hipGetErrorString(e)); }
  // finish: the tiles' pairs in tile order, an off-diagonal tile for its mirror image too
  double s1 = 0.0, s2 = 0.0;
  size_t t = 0;
  for (int ti = 0; ti < nt; ++ti)
    for (int tj = ti; tj < nt; ++tj, ++t) {
      const double w = tj == ti ? 1.0 : 2.0;
      s1 += w * part[2 * t]; s2 += w * part[2 * t + 1];
    }
  long long zeros = 0;
  for (int64_t i = 0; i < n; ++i) zeros += zr[(size_t)i];
  sums[0] = s1; sums[1] = s2; sums[2] = (double)zeros; sums[3] = (double)n;
  return 0;
}
