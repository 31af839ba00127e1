// base.inc -- errors, environment knobs, profile classes (inside the anonymous namespace)
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(x)                                                                              \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) return fail(-2, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define NCCL_TRY(x)                                                                             \
  do {                                                                                          \
    ncclResult_t r_ = (x);                                                                      \
    if (r_ != ncclSuccess) return fail(-3, "%s failed: %s (%s:%d)", #x, ncclGetErrorString(r_), __FILE__, __LINE__); \
  } while (0)
#define TRY(x)            \
  do {                    \
    int rc_ = (x);        \
    if (rc_ != 0) return rc_; \
  } while (0)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

// ---- environment of the library (INTEGRATION.md section D lists every name; each has a parity test) ------------------------------
// Product knobs, read when a handle is created: GANMF_MFMA, GANMF_MULTI, GANMF_X3KG, GANMF_SCORE_PRESPLIT, GANMF_SPARSE,
// GANMF_SPARSE_D, GANMF_FORCE_COLLECTIVES, GANMF_LANE_EVENT_FENCE, GANMF_DEBUG_PLAN, and GANMF_TUNE = "key=value,..." with the
// GEMM-plan overrides the kernel tests use to reach a variant at a small shape: tile (64 | 128), ring (2 | 3 | 4), kg (1 | 2 | 4),
// nsplit, tile_order (0 | 1 | 2), persist (-1 auto | 0 | 1), score_product (ganmf_bench_scores times the whole product),
// gram (K loop of ganmf_score_similarity's Gram product: 1 exact three-way bf16 split, the default | 0 plain fp32 MFMA).
// The alternatives that were measured slower and that no planner picks are not in the library (profiles/one_path.md lists them with
// the notes that hold their measurements).
int tune_env_int(const char* key, int dflt) {
  const char* s = getenv("GANMF_TUNE");
  if (!s) return dflt;
  const size_t n = strlen(key);
  while (*s) {
    while (*s == ',' || *s == ' ') ++s;
    if (!strncmp(s, key, n) && s[n] == '=') return atoi(s + n + 1);
    while (*s && *s != ',') ++s;
  }
  return dflt;
}
// K-loop arithmetic: GANMF_MFMA = f32 | bf16x3 | bf16 overrides the handle's choice (tests, A/B timing)
constexpr int MFMA_DEFAULT = MFMA_AUTO;
int env_mfma_mode(int dflt) {
  const char* v = getenv("GANMF_MFMA");
  if (!v || !*v) return dflt;
  if (!strcmp(v, "auto")) return MFMA_AUTO;
  if (!strcmp(v, "f32")) return MFMA_F32;
  if (!strcmp(v, "bf16x3")) return MFMA_BF16X3;
  if (!strcmp(v, "bf16")) return MFMA_BF16;
  if (!strcmp(v, "f16")) return MFMA_F16;
  return dflt;
}

constexpr int ADAM_GRID = 1024;
// The fused-Adam weight-gradient GEMMs under MFMA_AUTO: 64 x 64 tiles on the staged split-bf16 loop (the two [~1000 x ~3700 x 2B] TN
// GEMMs run 10 % faster there than on the fp32 MFMA, +2.7 % steps/s) with 32-deep K-tiles -- 24 KiB of LDS per workgroup: six co-resident
// workgroups hide the theta / m / v round trip of each other (33.6 / 28.8 us against 37.2 / 32.0 at 64)
constexpr int FUSED_MODE = MFMA_BF16X3, FUSED_TILE = 64, FUSED_BK = 32;

// profiling: kernel classes
enum Tag : int {
  T_DENSIFY, T_GEMM_GEN, T_RED_GEN, T_GEMM_ENC, T_RED_ENC, T_GEMM_DEC, T_RED_DEC, T_DCOEF, T_GEMM_DE, T_RED_DE,
  T_GEMM_GWD, T_RED_GWD, T_GEMM_GWE, T_RED_GWE, T_ADAM_D, T_GEMM_DF, T_RED_DF, T_GEMM_GUB, T_RED_GUB, T_GEMM_GV,
  T_RED_GV, T_ADAM_V, T_ADAM_U, T_MULTIRED, T_ALLREDUCE, T_SCORE_GEMM, T_RED_SCORE, T_DIS_FWD, T_RED_DIS_FWD, T_DIS_HEAD,
  T_DIS_GW, T_RED_DIS_GW, T_DIS_BWD, T_RED_DIS_BWD, T_FRONT, T_GWD_RED, T_PAIR, T_DE_DCOEF, T_WPAIR,
  T_COLL_WE, T_COLL_WD, T_COLL_V, T_JOIN_WE, T_JOIN_WD, T_JOIN_V, T_SIM_GRAM, T_SIM_AUX, T_EVAL_GROUPS,
  T_SVD_SPMM, T_SVD_GRAM, T_SVD_GRAM_RED, T_SVD_APPLY, T_SVD_APPLY_RED, T_SVD_CHOL, T_SVD_EIG, T_SVD_GLUE,
  T_NMF_SPMM, T_NMF_GRAM, T_NMF_GRAM_RED, T_NMF_MU_ROWS, T_NMF_CD_ROWS, T_NMF_SAMPLED, T_NMF_REDUCE,
  T_KNN_FIT, T_KNN_PACK, T_KNN_SCORE, T_P3_ROWS, T_P3_NORMALIZE, T_P3_COLUMNS, T_COUNT
};
const char* const kTagName[T_COUNT] = {
  "densify_rows+gather", "gemm_generator[B,k]x[N,k]^T", "reduce_generator", "gemm_encode[2B,N]x[N,e]",
  "reduce_encode", "gemm_decode[2B,e]x[e,N]", "reduce_decode+mse", "d_coef+scale", "gemm_dE[2B,N]x[e,N]^T",
  "reduce_dE", "gemm_gWd[2B,e]^Tx[2B,N]", "reduce_gWd", "gemm_gWe[2B,N]^Tx[2B,e]", "reduce_gWe", "adam_dense_D",
  "gemm_dF[B,e]x[N,e]^T", "reduce_dF", "gemm_gUb[B,N]x[N,k]", "reduce_gUb", "gemm_gV[B,N]^Tx[B,k]", "reduce_gV",
  "adam_dense_V", "adam_rows_U", "multi_reduce", "rccl_allreduce", "gemm_scores", "reduce_scores",
  "gemm_dis_layer_fwd", "reduce_dis_layer_fwd", "dis_head", "gemm_dis_gW", "reduce_dis_gW", "gemm_dis_bwd",
  "reduce_dis_bwd", "gemm_generator[B,k]x[N,k]^T + CSR rows (one launch)", "gemm_gWd[2B,e]^Tx[2B,N] + reduce_dE (one launch)",
  "gemm_gUb[B,N]x[N,k] + gemm_gV[B,N]^Tx[B,k] (one launch)", "gemm_dE[2B,N]x[e,N]^T + d_coef (one launch)",
  "gemm_gWd + gemm_gWe, fused Adam (one launch)",
  // data-parallel step: reduce-scatter + all-gather of one replicated tensor (side lane), and the time the MAIN lane spent
  // waiting at the join in front of that tensor's next reader (the exposed part of the collective)
  "collective_We (reduce-scatter + all-gather)", "collective_Wd (reduce-scatter + all-gather)",
  "collective_V (reduce-scatter + all-gather)", "join_wait_We (main lane)", "join_wait_Wd (main lane)", "join_wait_V (main lane)",
  // ganmf_score_similarity: the symmetric Gram product with its statistics, and the row normalisation / block means around it
  "gram_similarity[n,W]x[n,W]^T + stats", "similarity_normalize / pool",
  // ganmf_evaluate_groups: the per-user metric values and their sums per group of users
  "eval_groups: per-user metrics / group sums",
  // ganmf_pure_svd: sparse x dense panel, Gram and apply products with their split-K sums, Cholesky + inverse, Jacobi, select / finish
  "svd_spmm[rows,nnz]x[cols,l]", "svd_gram[n,l]^Tx[n,l]", "reduce_svd_gram", "svd_apply[n,l]x[l,.]", "reduce_svd_apply",
  "svd_cholesky_inverse[l,l]", "svd_jacobi[l,l]", "svd_select / finish",
  // ganmf_nmf_*: sparse x factor, the Gram matrix of a factor with its split-K sum, the two row solvers, the sampled products of the
  // Kullback-Leibler loss, column sums / traces / totals (the item-similarity classes keep the end of the enum: tests/test_p3_dropin.py)
  "nmf_spmm[rows,nnz]x[cols,k]", "nmf_gram[n,k]^Tx[n,k]", "reduce_nmf_gram", "nmf_mu_rows", "nmf_cd_rows", "nmf_sampled[nnz]",
  "nmf_colsum / dot / sum",
  // ganmf_itemknn_fit: one similarity row and its top-k per item, the columns packed by neighbour id; the sparse scoring product
  "itemknn_fit: similarity row + top-k", "itemknn_pack", "itemknn_scores[n,items]x W",
  // ganmf_p3_fit: one row of the random walk and its top-k per source item, the row normalisation, the top-k per target item
  "p3_rows: walk row + top-k", "p3_normalize", "p3_columns: column top-k / transpose"};
static_assert(T_COUNT <= GANMF_PROF_MAX, "ganmf_profile_read's callers size their buffer by GANMF_PROF_MAX");

struct ProfRec { int tag; hipEvent_t a, b; double flops, bytes; };

