// handle.inc -- the loopback communicator's group state and struct ganmf_handle
// (a fragment of libganmf_hip.so's single translation unit: included by ganmf_hip.hip, in its order)

// A parameter with its Adam moments and best-snapshot twin.  g is a view: a slice of the handle's gD for the tensors whose gradients
// are reduced together, or the tensor's own g_own (alloc_tensor's grad_separate).
struct Tensor {
  int rows = 0, cols = 0, ld = 0;
  DevBuf<float> p, m, v, best, g_own;
  float* g = nullptr;
  size_t cap = 0;          // allocated elements: padded() rounded up to world_size equal slices of a multiple of 64 floats
  size_t padded() const { return (size_t)rows * ld; }
  size_t count() const { return (size_t)rows * cols; }
};

// ---- in-process loopback communicator: group state (see allreduce_local) ----
constexpr int LOCAL_MAX_WORLD = 8;
struct LocalPtrs { float* p[LOCAL_MAX_WORLD]; };
enum LocalOp : int { LOCAL_ALLREDUCE = 0, LOCAL_REDUCE_SCATTER = 1, LOCAL_ALLGATHER = 2 };
// count = elements of the whole buffer (world slices for the scatter / gather forms); sums run in rank order
__global__ void local_collective_kernel(LocalPtrs b, int world, size_t count, int op) {
  const size_t slice = count / (size_t)world;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    if (op == LOCAL_ALLGATHER) {
      const float v = b.p[i / slice][i];           // the owner's copy of its slice
      for (int r = 0; r < world; ++r) b.p[r][i] = v;
      continue;
    }
    float s = b.p[0][i];
    for (int r = 1; r < world; ++r) s += b.p[r][i];
    if (op == LOCAL_ALLREDUCE) { for (int r = 0; r < world; ++r) b.p[r][i] = s; }
    else b.p[i / slice][i] = s;                    // reduce-scatter: only the owner of the slice receives the sum
  }
}
struct LocalGroup {
  std::mutex mu;
  std::condition_variable cv;
  int world = 0, dev = -1, arrived = 0, joined = 0;
  long long generation = 0;
  size_t count = 0;
  int op = 0;
  bool failed = false;
  LocalPtrs bufs{};
};

// one side of the handle's weighted sparse matrix (ganmf_als_set_confidence): CSR over that side's rows -- the ALS confidences, or
// the URM itself for ganmf_pure_svd
struct AlsSide : DevCsr {
  DevBuf<float> conf;
  bool canonical = false;      // every row's columns ascend without repeats (what the GANMF_MODEL_ITEMSIM entries need)
};

// a compact similarity matrix with its values: the one a GANMF_MODEL_ITEMSIM handle holds, and the temporaries between two passes of a fit
struct SimCsr : DevCsr {
  DevBuf<float> val;
  void drop() { DevCsr::drop(); val.reset(); }
};

// The profiles an SGD trainer draws its samples from, on the device (profiles_upload / profiles_drop of lib/sgd_train.inc; draw_kernel):
// users x items in CSR with ascending items, the stored values where the trainer reads them, and the users with 0 < |profile| < n_items
struct SampleProfiles : DevCsr {
  DevBuf<double> ratings;         // FunkSVD's; else null
  DevBuf<int> eligible;           // [n_eligible] ascending
  int n_eligible = 0;
};

// SLIM-BPR training state of a GANMF_MODEL_ITEMSIM handle (ganmf_slim_bpr_init; slim_bpr.hpp): S and the optimiser state in float64,
// the profiles the samples are drawn from and summed over (a copy of side 0's pattern, or the caller's), and what the host carries
// from call to call: the epoch counter of the sampler and Adam's beta powers
struct SlimState {
  bool ready = false;
  int symmetric = 0, sgd = 0;
  double lr = 0, li = 0, lj = 0, gamma = 0, b1 = 0, b2 = 0, b1_pow = 0, b2_pow = 0;
  uint64_t seed = 0;
  int64_t epoch = 0;
  size_t cells = 0;
  DevBuf<double> S, st0, st1;
  SampleProfiles profiles;
};

// SGD matrix-factorisation training state of a GANMF_MODEL_MF handle (ganmf_mf_sgd_init; mf_sgd.hpp).  P holds three blocks of `block`
// float64 values -- the parameters, st0, st1 -- each laid out [W: U k | H: N k | USER_bias: U | ITEM_bias: N | GLOBAL_bias: 1]; the
// profiles the samples are drawn from with their stored values, phase 1's per-sample terms of one batch, and what the host carries
// from call to call: the epoch counter of the sampler and Adam's beta powers (one multiplication per BATCH)
struct MfSgdState {
  bool ready = false;
  int algo = 0, k = 0, use_bias = 0, sgd = 0;
  double lr = 0, user_reg = 0, item_reg = 0, pos_reg = 0, neg_reg = 0, bias_reg = 0, quota = 0;
  double gamma = 0.995, b1 = 0.9, b2 = 0.999, b1_pow = 0.9, b2_pow = 0.999;      // (fit() never forwards them: fixed)
  uint64_t seed = 0;
  int64_t epoch = 0;
  size_t block = 0;
  DevBuf<double> P;
  SampleProfiles profiles;
  DevBuf<double> terms;
};

// The generator CFGAN and CAAE share (profile_mlp.inc): an MLP from a dense profile row [N] through Lg hidden layers of g units back to
// [N], every bias folded into its tensor as the last row and fed by a ones column of the layer's input.
struct ProfileMlp {
  int g = 0, Lg = 0, act = 0, ldg = 0;      // width, depth, hidden activation
  int out_act = -1;                         // activation of the output layer (-1: none; CAAE: the sigmoid)
  std::vector<Tensor> Gl;        // l = 0: [N + 1, g] (row N the bias); l > 0: [g + 1, g]
  Tensor Go;                     // [g + 1, N] (row g the bias), leading dimension ldN
  std::vector<DevBuf<float>> Hl;       // hidden outputs of a training batch [rows, ldg] with the ones column at g
  // scratch of a block of sc_rows scored rows: dense profiles, two hidden blocks (the layers alternate), one output block
  DevBuf<float> sc_C, sc_H0, sc_H1, sc_F;
  size_t sc_rows = 0;
  std::vector<Tensor*> tensors() {
    std::vector<Tensor*> v;
    for (auto& t : Gl) v.push_back(&t);
    v.push_back(&Go);
    return v;
  }
};

// CFGAN state of a GANMF_MODEL_CFGAN handle (ganmf_cfgan_init; step_cfgan.inc).  The discriminator lives in the handle's DisGANMF
// members (Wl, Wo, Al, dz0, dz1, dlogit; Wl[0] is [2N + 1, e]: condition rows, input rows, bias row); the generator, the masks and the
// step's work buffers live here.  Bm = max(d_batch, g_batch) rows.
struct CfganState {
  bool ready = false;
  int d_batch = 0, g_batch = 0, scheme = 0, Bm = 0, ldx = 0, words = 0;
  float zr_coef = 0.f;
  uint64_t seed = 0;
  ProfileMlp gen;
  DevBuf<float> C, fake, dfake, DX, dh0, dh1;
  DevBuf<float> zr_part, loss_rows, sq, loss_dev;
  DevBuf<unsigned> planes;       // [2][U][words]: CFGAN_PLANE_ZR, CFGAN_PLANE_PM
  DevBuf<int> k_rows;            // [U]
  DevBuf<float> cache;           // item-mode scoring: the transposed G(all rows) [N, ld(U)] as of cache_version
  long long cache_version = -1;
};

// CAAE state of a GANMF_MODEL_CAAE handle (ganmf_caae_init; step_caae.inc).  The discriminator's embeddings P, Q are the handle's
// factor tensors Ue [U, k] and V [N, k]; its item bias, the two generators (gen[0] = G, gen[1] = G': built alike, sigmoid on every
// layer), the epoch's draws and the steps' work buffers live here.
struct CaaeState {
  bool ready = false;
  int Bm = 0, n_s = 0, words = 0, d_bsize = 0;
  float lmbda = 0.f, beta = 0.f, lr = 0.f;
  uint64_t seed = 0;
  ProfileMlp gen[2];
  Tensor bias;                   // disc_item_bias [1, N]
  DevBuf<int> k_rows;            // [U] size of Nu per user
  // the epoch's state: both CDFs [U, ldN], the user of every stored interaction, the shuffled order and its triples
  DevBuf<float> cdf[2];
  DevBuf<int> iu;                // [nnz] row of CSR position e
  const void* iu_src = nullptr;  // the indptr it was formed from
  DevBuf<int> perm, tu, ti;      // [nnz]: CSR position, user and item of every position of the shuffled order
  // recorded draws of the last epoch, per pass / step slot (ganmf_caae_get_draws)
  DevBuf<int> neg;               // [passes][2][nnz]
  DevBuf<int> users;             // [2][steps][Bm]
  DevBuf<unsigned> nu;           // [steps][Bm * words]
  DevBuf<int> items;             // [2][steps][Bm * n_s]
  int step_slots = 0, rec_passes = 0, rec_steps[2] = {0, 0};
  long long rec_nnz = 0;
  // explicit triples of a single D-step, the gathered rows and per-triple values of the step in flight
  DevBuf<int> xt;                // [3][d_bsize]
  DevBuf<int> first;             // [U + N] CaaeDP::first: 0x7f7f7f7f between steps
  DevBuf<int> xu, xi;            // [Bm], [Bm * n_s]: users and policy items of a single step or draw entry
  DevBuf<unsigned> xn;           // [Bm * words]: its Nu planes
  DevBuf<float> Pg, Qi, Qj, coef, lt, rt;
  // generator step: profiles, outputs of G and G', batch CDF, d loss / d z of the output layer, hidden gradients, per-row parts
  DevBuf<float> C, R, Rp, cdfb, dz, dh0, dh1;
  DevBuf<float> lse, reward, la, ae, sq, loss_dev;
  DevBuf<float> lse_all;         // [U] log sum exp(r) of the all-users CDF pass
};

struct ganmf_handle {
  ganmf_cfg cfg;
  int dev = 0;
  hipStream_t st = nullptr;
  hipStream_t st2 = nullptr;             // side lane: independent kernels overlap the main lane
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mid = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;   // ganmf_stream_timer
  hipEvent_t ev_we = nullptr, ev_wd = nullptr;   // data-parallel: "the side lane has finished updating We / Wd" (dp_mark / dp_join)
  int U = 0, N = 0, k = 0, e = 0, B = 0;
  int ldN = 0, ldk = 0, lde = 0;
  // DisGANMF (model 1): hidden layers W_l_ext and the output unit; see the DisGANMF section below
  int L = 0, act = 0;
  std::vector<Tensor> Wl;   // l = 0: [N+2, e] rows 0..N-1 profile weights, row N bias, row N+1 the float(uid) weight; l > 0: [e+1, e]
  Tensor Wo;                // [1, e+1]: output kernel (e) then output bias
  std::vector<DevBuf<float>> Al;   // layer outputs [2B, lde] with the ones column at e
  DevBuf<float> dz0, dz1, dlogit;
  Tensor We, Wd, Ue, V;   // We = We_ext [N+1, e] (row N = encoder bias), Wd = Wd_ext [e+1, N] (row e = decoder bias)
  DevBuf<float> gD;     // contiguous [gWe_ext | gWd_ext] (one all-reduce)
  size_t gD_elems = 0;
  // CSR
  DevCsr urm;
  DevBuf<float> data;
  bool has_urm = false;
  bool sparse_g = false;   // SURVEY 8(f)-3: generator steps take the real rows' encodings from a CSR row-sum (no densify of X)
  bool sparse_d = false;   //               discriminator steps too: Er from the CSR rows, X subtracted from the reconstruction through a CSR
                           //               lookup in the decode epilogue, X^T.dE_r added to the encoder gradient from the CSC matrix
  DevCsr csc;                        // CSC form of the same matrix (sparse_d): column j = the rows that store item j, ascending
  DevBuf<float> csc_val;
  DevBuf<float> sp_rows;             // [N + CSC_BIAS_PARTS, lde]: X^T . dE_r of the step in flight (csc_rows_kernel)
  // epoch schedule
  DevBuf<int> perm;         // [3U] device: the epoch's permutation, then (pos = perm + U) its inverse, then pos_step
  PinnedBuf<int> stage_i;   // pinned host staging (ensure_stage)
  PinnedBuf<float> stage_f;
  // Views into buffers owned elsewhere, never freed: pos, pos_step (perm), XF (XF_own or a block of XF_pass), Ub / gUb (Ub_own /
  // gUb_own, Ub_sched or a lazy chunk), d_parts / g_parts / d_arena / g_arena (parts_all), dis_slot (an arena), Tensor::g
  int* pos = nullptr;
  float *XF = nullptr, *Ub = nullptr, *gUb = nullptr;
  // minibatch work buffers
  DevBuf<float> E, Es, Dl, dE, dF;
  // staged discriminator pass (stage_pass, step_ganmf.inc): U and V are frozen for the whole pass (GANMF.py:176-189), so the CSR row
  // expansion and the generator product of ALL its full minibatches run once, in front of it, into one [real ; generated] block of 2B rows
  // per minibatch; XF then points at the block of the step in flight (XF_own: the handle's own 2B-row buffer)
  DevBuf<float> XF_own;
  DevBuf<float> XF_pass;
  DevBuf<float> Ub_pass;                 // U rows of the pass in schedule order (only when the generator product does not gather them itself)
  bool skinny = true;                    // GANMF_TUNE=skinny=0: K <= 64 products stay on the tiled MFMA kernels
  int bf16w = 1;                         // GANMF_TUNE=bf16w=0: products that would run as two K slices per 64 x 64 tile stay that way (2: the 64 x 32 kernel wherever eligible)
  bool skinny_n = true;                  // GANMF_TUNE=skinny_n=0: N <= 32 products behind a long K stay on the tiled MFMA kernels
  bool pass_stage = true;                // GANMF_TUNE=pass_stage=0: every step expands its own rows
  bool pass_buffers_tried = false;       // prealloc_pass_buffers ran (first training call)
  bool x_staged = false;                 // the generator step in flight finds its real rows (X half of its block of XF_pass) staged: h->XF points at the block
  bool front_staged = false;             // the discriminator step in flight finds X, F (and its lr_t slot) staged
  int tab_cap = 0;                       // lr_t slots per table from scal[S_TAB] (four tables: discriminator / generator passes, each alternating)
  // generator pass with the all-rows update of U once per pass (kernels.hpp adam_rows_advance_kernel / adam_rows_flush_kernel; g_reg == 0)
  bool lazy_rows = true;                 // GANMF_TUNE=lazy_rows=0: adam_rows_kernel over all rows in every generator step
  bool lazy_pass = false;                // the generator step in flight belongs to such a pass
  int g_alpha = S_ALPHA_G;               // scalar slot holding lr_t of the generator step in flight
  DevBuf<float> Ub_own;                  // the handle's own [B, ldk] minibatch embeddings (Ub points into Ub_sched during a lazy pass)
  DevBuf<float> gUb_own;
  DevBuf<float> Ub_sched;                // [n, ldk] embeddings of the scheduled rows as their step will read them
  int* pos_step = nullptr;               // [U] device: step index of every schedule position (perm + 2U)
  std::vector<DevBuf<float>> lazy_chunks;      // gUb (slabs) of every step of the pass: bump-allocated, kept across passes
  size_t lazy_chunk = 0, lazy_used = 0;
  std::vector<LazyStep> lazy_steps;
  int lazy_step = 0;                     // index of the generator step in flight within its pass
  PinnedBuf<LazyStep> lazy_stage;        // pinned host staging of the table, two halves (passes alternate)
  DevBuf<LazyStep> lazy_tab;             // device copy of lazy_steps
  DevBuf<float> zero_page;
  DevBuf<float> slab;
  DevBuf<float> slab2;                   // split-K workspace of the side lane
  float* slab2_lent = nullptr;           // view: a block of the pass arena that stands in for slab2 during one run_gemm (gen_update)
  size_t slab2_lent_elems = 0;
  int x3kg = 7;                   // GANMF_X3KG bits: 16-wave split-bf16 loop for the plans of the 16-wave fp32 ring kernel (1 NT, 2 K-major B), 4: its one-piece form for bf16 / fp16 plans
  DevBuf<float> rs;
  DevBuf<float> scal;
  DevBuf<float> sqp;     // [2][max_tiles]
  int sqp_stride = 0;
  int reg_cap = 0;
  bool dis_colsum_pending = false;      // this discriminator step's column sums (ColSumP dis_colsum) ride in the layer-0 gradient GEMM's launch (dis_d_step)
  ColSumP dis_colsum{};
  bool dis_uid_done = false;    // this discriminator step's dis_dz_top_kernel formed the gradient of W_0_ext's float(uid) row and updated it (dis_d_step)
  int dis_cap = 0;              // DisGANMF: floats per segment of a step's arena slot (5 + L segments, finish_dis_parts_kernel)
  float* dis_slot = nullptr;    //           slot of the step in flight
  std::vector<char> dis_fused;  // DisGANMF, per layer: this step's update ran in the epilogue of its gradient GEMM (dis_backprop_hidden)
  std::vector<int> dis_regn;    //           and left this many sum(theta^2) partials
  bool defer_gub = true;  // the split-K slabs of gUb are summed by adam_rows_kernel (no reduce launch)
  int multi = 31;         // combined launches (gemm_multi.hpp), bit 0: generator GEMM + CSR row expansion, bit 1: gUb + gV,
                          // bit 2: slab sum of dE inside the gWd launch, bit 3 (with bit 2): d_coef inside the dE launch,
                          // bit 4 (with bit 2): gWd + gWe in one launch behind a stand-alone slab sum of dE (GANMF_MULTI)
  DevBuf<float> V_alt;   // second parameter buffer of item_embeddings: the fused gV update is written there while gUb
                          // still reads the old V in the same launch; swapped with V.p after the launch
  bool dis_fuse_hidden = true;   // DisGANMF: also for the hidden layers l > 0 (GANMF_DIS_FUSE_HIDDEN)
  DevBuf<float> parts_all;                       // ONE allocation: [d_parts | g_parts | d_arena | g_arena], packed per call (parts_begin)
  float *d_parts = nullptr, *g_parts = nullptr;  // [steps][4]
  DevBuf<float> colbuf;                          // [cap] one column of d_parts on its way through an all-reduce
  float *d_arena = nullptr, *g_arena = nullptr;  // [cap][4][reg_cap] per-step block partials (GANMF), reduced once per epoch
  // recommend(): URM_train in evaluation orientation for the seen-item mask, top-k outputs
  DevCsr seen;
  // score filter (ganmf_set_score_filter): byte per score column (1 = computed), and whether cold rows are masked
  DevBuf<unsigned char> item_mask;
  int64_t item_mask_w = 0;             // 0: no item filter; else one past the largest listed item
  bool mask_cold = false;
  // ignore list (ganmf_set_items_to_ignore): byte per score column (1 = ignored) on the host, beside the host copy of the score filter's
  // bytes; while a list is set, rank_mask holds the keep-mask everything that RANKS uses -- (no item filter, or listed by it) and not
  // ignored -- formed by whichever of the two setters ran last.  ganmf_scores keeps reading item_mask.
  std::vector<unsigned char> filter_host, ignore_host;
  int64_t ignore_w = 0;                // 0: no ignore list; else one past the largest ignored item
  DevBuf<unsigned char> rank_mask;
  DevBuf<int> topk_items;          // the two top-k outputs hold the same count: topk_vals is grown last, so its cap is what both hold
  DevBuf<float> topk_vals;
  // ganmf_set_item_diversity: the [div_w, div_w] item diversity matrix of ganmf_evaluate_diversity, resident until replaced
  DevBuf<float> div_mat;
  int64_t div_w = 0;
  // ganmf_evaluate(): URM_test in evaluation orientation (sorted rows) with the DCG gains, work buffers
  DevCsr test;
  DevBuf<double> test_gain;
  DevBuf<double> eval_buf;         // disc | ideal_cum | block partials
  // ganmf_evaluate_full(): rating per stored test entry (dropped by every ganmf_set_test_csr), the two per-item weights of the
  // evaluation width, and work buffers (per-row RMSE, [n_cutoffs, W] counts)
  DevBuf<float> test_rating;
  bool test_rating_ok = false;
  DevBuf<double> eval_w;           // novelty | popularity, eval_w_width each
  int64_t eval_w_width = 0;
  DevBuf<float> eval_rmse;
  DevBuf<unsigned> eval_counts;
  // ganmf_evaluate_groups(): members of every group | their begin offsets (the per-user values and the group sums live in eval_buf)
  DevBuf<int> eval_grp;
  // ganmf_set_candidates_csr: per-row candidate lists (evaluation orientation, rows sorted and unique) for cand_topk_kernel;
  // the host keeps the row pointers to size a launch's LDS and to refuse a row over GANMF_CANDIDATES_MAX_PER_ROW without launching
  DevCsr cand;
  std::vector<long long> cand_indptr_host;
  // scoring scratch
  DevBuf<int> sc_ids;
  DevBuf<float> sc_rows, sc_out;
  DevBuf<unsigned> sc_pa, sc_pb;                    // bf16 x 3 planes of the scored rows / of the other factor (gemm_bf16p.hpp)
  const float* sc_pb_src = nullptr;                 // what sc_pb holds: the planes of this parameter buffer ...
  long long sc_pb_version = -1, param_version = 0;  // ... as of this parameter version (bumped by training, set_tensor, restore_best)
  int sc_pb_rows = 0;
  // ganmf_score_similarity (gram_stats.hpp): the similarity matrix [n, ld(n)] (only when the matrix or its block means are asked for), the
  // block means, the per-tile (sum d, sum d^2) pairs and the zero-row flags; grown on demand.  The normalised rows live in sc_out.
  DevBuf<float> sim_mat, sim_pool;
  DevBuf<double> sim_part;
  DevBuf<int> sim_zero;
  // ganmf_discriminate (disc_rows.hpp): block buffers of its own, grown on demand -- the ids, the input block [blk, ldN] (generated rows,
  // or DisGANMF's expanded rows), the gathered embeddings [blk, ldk], the codes / layer outputs [blk, lde] (two: the layers alternate), the
  // per-(row, column tile) partials and the values.  The step's buffers, the staged-pass state and the beta powers are never touched.
  DevBuf<int> dr_ids;
  DevBuf<float> dr_X, dr_Ub, dr_E, dr_A;
  DevBuf<double> dr_part, dr_val;
  int64_t disc_block = 0;                           // ganmf_set_discriminate_block: rows per block of the call's loop (0: a quarter of the free memory)
  // ganmf_als_half_sweep (als_rows.hpp): the confidence matrix in both orientations, G = Y^T Y [k, ldk], and the failure words
  // [1 + max(U, N)] (word 0: any row of the call, word 1 + u: row u)
  AlsSide als[2];
  DevBuf<float> als_G;
  DevBuf<int> als_bad;
  // GANMF_MODEL_ITEMSIM (itemknn_rows.hpp): the item similarity matrix W by target item -- column i of the reference's W_sparse is
  // knn_nbr / knn_val [knn_indptr[i], knn_indptr[i + 1]) -- from ganmf_itemknn_fit or ganmf_set_item_similarity; knn_dense: the dense
  // profiles [rows, ld] of the scoring route for catalogues above one workgroup's LDS, grown on demand.  The one held matrix may
  // instead be a USER similarity (knn_user = 1; userknn_rows.hpp): W_sparse [U, U] by row -- row u is knn_nbr / knn_val
  // [knn_indptr[u], knn_indptr[u + 1]) -- from ganmf_userknn_fit or ganmf_set_user_similarity
  SimCsr knn;                // knn.indices, knn.val: knn_nbr, knn_val of the comment above
  int64_t knn_nnz = -1;      // -1: no matrix held
  int knn_user = 0;          // the held matrix: 0 item x item by target item, 1 user x user by row
  DevBuf<float> knn_dense;
  SlimState slim;                                   // ganmf_slim_bpr_* (slim_bpr.hpp)
  MfSgdState mfs;                                   // ganmf_mf_sgd_* (mf_sgd.hpp)
  CfganState cf;                                    // ganmf_cfgan_* (cfgan_masks.hpp, cfgan_rows.hpp)
  CaaeState ca;                                     // ganmf_caae_* (caae_sample.hpp, caae_rows.hpp)
  // ganmf_pure_svd (svd_rows.hpp): the two panels [max(U, N), svd_ldl] the iteration alternates between, the Gram matrix and the
  // inverse Cholesky factor [svd_ldl, svd_ldl], the [svd_ldl, ldk] matrix W of the final products, lambda [svd_ldl] | sigma [ldk],
  // and the failure words (SvdCholP::flag).  Allocated by the first call, regrown by a call with a wider n_random.
  DevBuf<float> svd_P[2];
  DevBuf<float> svd_G, svd_X, svd_Wl, svd_lam;
  DevBuf<int> svd_flag;
  int svd_ldl = 0;
  // ganmf_nmf_* (nmf_rows.hpp): the denominator and numerator panels [max(U, N), ldk], the Gram matrices of both factors [2][ldk, ldk], the value
  // array of the sampled products [nnz], the two column-sum vectors [2][ldk], the per-row float64 values [2 max(U, N)], the partial
  // sums [NMF_PARTS], the scalars [4 + iterations] and the permutations of a call; allocated by the first call, grown on demand
  DevBuf<float> nmf_den, nmf_num, nmf_G, nmf_q, nmf_vec;
  DevBuf<double> nmf_rowd, nmf_part, nmf_scal;
  DevBuf<int> nmf_perm, nmf_rowidx;                    // nmf_rowidx [2][nnz]: the row of every CSR position of both sides
  DevBuf<double> nmf_errp;                             // [chunks, 2] divergence sums of nmf_sampled_kernel
  int gram_arith = 1;                               // GANMF_TUNE gram: 1 (default, the faster one measured) the exact three-way bf16 split, 0 the plain fp32 MFMA body
  bool score_presplit = true;                       // GANMF_SCORE_PRESPLIT: many-tile scoring products on the pre-split persistent kernel
  // RCCL
  ncclComm_t comm = nullptr;
  bool has_comm = false;
  // ganmf_comm_abort ran on the RCCL communicator (ncclCommAbort frees it: no ncclCommDestroy afterwards, and no collective may be enqueued on
  // it any more).  Written by the aborting thread, read by the handle's own thread: atomic, and every use of `comm` (the collective wrappers,
  // ganmf_comm_info, the abort itself) happens under comm_mu behind a check of the flag, so an enqueue can never race the free.
  std::atomic<bool> comm_aborted{false};
  std::mutex comm_mu;
  std::shared_ptr<LocalGroup> local;   // in-process loopback communicator (ganmf_comm_init_local)
  int d_alpha = S_ALPHA_D;             // scalar slot holding lr_t of the discriminator step in flight (alternates in data-parallel runs)
  int side_pending = 0;                // data-parallel: PEND_* bits of the replicated tensors the side lane still updates (dp_join
                                       // before their next use on the main lane)
  int wgrad_xb = 16;                   // GANMF_TUNE wgrad_xb: gWd of the paired launch in XCD-blocked tile order, bands of this many tile rows (0: list order)
  int adam_touch = 1;                  // GANMF_TUNE adam_touch: gV + Adam(V) touches its tile's theta / m / v lines in front of the K loop (GemmP::adam_touch, adam_touch_for)
  bool gub_x3 = false;                 // gV runs on the staged kernel (wide V: >= two tiles per CU), so gUb can never pair with it: its stand-alone plan may take
                                       // the 16-wave split-bf16 loop like every other NN product (gen_update; 46 -> 38 us at the configs[3] shard)
  int g_rows_staged = 1;               // GANMF_TUNE g_rows_staged: the generator passes read their real rows from the blocks staged in front of the call
                                       // (1: where the per-step row expansion is a launch of its own, 2: wherever possible, 0: never)
  long long fork_armed_at = 0;         // launch_count() when fork_arm() handed ev_fork to the next launch
  bool force_coll = false;             // GANMF_FORCE_COLLECTIVES=1: a one-rank communicator still issues its (in-place) reduce-scatter /
                                       // all-gather calls, so that the RCCL call sites execute on a one-GPU box (tests, bench)
  // tuning knobs (environment: GANMF_TILE, GANMF_RING, GANMF_NSPLIT; 0 = cost model decides)
  GemmTune tune;
  bool debug_plan = false;
  std::vector<long long> seen_plans;
  // profiling
  bool prof = false;
  std::vector<ProfRec> recs;
};

