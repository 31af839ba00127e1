/*
 * ganmf_hip.h — C ABI of libganmf_hip.so: the MI355X (gfx950) GANMF / DisGANMF training hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one interaction the reference has
 * with its numeric runtime (a TensorFlow-1.12 tf.Session); the reference site is cited per
 * function (paths relative to the reference repository root).  The Python host classes in
 * ganmf_amd/ bind exactly these symbols through ctypes; nothing else crosses the boundary.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every host buffer; the library copies in/out
 *     before returning; the handle owns all device memory, its HIP stream and (optionally) its
 *     RCCL communicator.
 *   - return value 0 = OK, negative = error; ganmf_last_error() returns a thread-local message.
 *     No exceptions cross the ABI and the library never calls exit().
 *   - a handle is driven by one host thread at a time; distinct handles are independent.
 *   - all floating point data are IEEE float32 (the reference's dtype, GANMF.py:108), ids int32
 *     (GANMF.py:109), CSR row pointers int64.
 *   - "training orientation": rows = the generator's users, columns = profile width.  In item
 *     mode the host passes URM^T (GANMF.py:32-36).
 */
#ifndef GANMF_HIP_H
#define GANMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GANMF_ABI_VERSION 2

typedef struct ganmf_handle ganmf_handle;

/* GANMF_MODEL_MF: a plain matrix-factorisation model (Base/BaseMatrixFactorizationRecommender.py:94-143: USER_factors, ITEM_factors).  The
 * handle holds only GANMF_T_USER_EMB / GANMF_T_ITEM_EMB (GANMF_SLOT_PARAM and GANMF_SLOT_BEST) and what scoring, recommendation and
 * evaluation need; emb_dim, batch_size and the learning rates are ignored (emb_dim and batch_size must still be >= 1).  The training
 * entries and ganmf_discriminate return -1 on it; every scoring, recommend, evaluate, snapshot and tensor entry works unchanged.  Its
 * factors come from ganmf_als_half_sweep, ganmf_pure_svd or ganmf_set_tensor. */
/* GANMF_MODEL_ITEMSIM: a similarity-matrix model (Base/BaseSimilarityMatrixRecommender.py:73-92: scores = URM_train[users] . W_sparse).
 * The handle holds no tensor at all: it holds the weighted URM in both orientations (ganmf_als_set_confidence) and the item similarity
 * matrix W (ganmf_itemknn_fit or ganmf_set_item_similarity).  num_factors, emb_dim and batch_size are ignored (each must still be >= 1).
 * ganmf_scores, ganmf_recommend, ganmf_evaluate, ganmf_evaluate_full, ganmf_evaluate_groups and ganmf_evaluate_diversity (candidates = 0),
 * the score filter, the ignore list and the seen / test uploads work unchanged: only the source of the score rows differs.  The
 * training, discriminator, tensor, snapshot, ALS, SVD, candidate and score-similarity entries return -1 on it with a message that
 * names the model, and enqueue nothing.  The enum gained a value; no structure or signature changed: GANMF_ABI_VERSION stays. */
/* GANMF_MODEL_CFGAN: CFGAN (GANRec/CFGAN.py): an MLP generator over the row's own profile and an MLP discriminator over [profile |
 * profile-shaped input], trained with per-epoch zero-reconstruction / partial-masking masks.  emb_dim, d_layers, d_act, d_lr, g_lr, d_reg
 * and g_reg of ganmf_cfg describe the discriminator and the two optimisers; batch_size is the larger of the two batch sizes;
 * num_factors, m and recon_coefficient are ignored (num_factors must still be >= 1); world_size must be 1 and the bf16 / fp16 MFMA flags
 * are refused.  ganmf_cfgan_init supplies the rest (below).  The handle holds no factor tensors.  The tensor, snapshot, seen / test
 * upload, ganmf_scores, ganmf_recommend, ganmf_evaluate* (candidates = 0), score filter, ignore list and score-similarity entries work
 * unchanged: only the source of the score rows differs (transposed = 0: G(profile of row id); transposed = 1: rows of the transposed
 * G(all rows), cached on the device until a parameter changes).  ganmf_train_epoch / _epoch_ragged / _step, ganmf_discriminate,
 * ganmf_als_half_sweep, ganmf_pure_svd, the item-similarity, P3 and SLIM entries, the candidate entries, ganmf_bench_scores and the two
 * communicator entries return -1 on it with a message that names the model.  The enum gained a value; no structure or signature changed: GANMF_ABI_VERSION stays. */
/* GANMF_MODEL_CAAE: CAAE (GANRec/CAAE.py): a pairwise discriminator over (user, positive item, negative item) triples -- embeddings P
 * [U, k], Q [N, k] and an item bias, held as the handle's two factor tensors and GANMF_T_CAAE_ITEM_BIAS -- and two sigmoid MLP generators G
 * and G' over the user's profile, all three trained by plain SGD.  Of ganmf_cfg only num_users, num_items, num_factors (at most
 * GANMF_CAAE_MAX_FACTORS), device and flags are read (emb_dim and batch_size must still be >= 1); world_size must be 1 and the bf16 /
 * fp16 MFMA flags are refused.  ganmf_caae_init supplies the rest (below).  The tensor, snapshot, seen / test upload, ganmf_scores,
 * ganmf_recommend, ganmf_evaluate* (candidates = 0), score filter, ignore list and score-similarity entries work unchanged with
 * transposed = 0: the score rows are sigmoid(G(profile of row id)).  Every entry that refuses a GANMF_MODEL_CFGAN handle refuses this one
 * too, with a message that names the model.  The enum gained a value; no structure or signature changed: GANMF_ABI_VERSION stays. */
enum { GANMF_MODEL_GANMF = 0, GANMF_MODEL_DISGANMF = 1, GANMF_MODEL_MF = 2, GANMF_MODEL_ITEMSIM = 3, GANMF_MODEL_CFGAN = 4, GANMF_MODEL_CAAE = 5 };
enum { GANMF_ACT_LINEAR = 0, GANMF_ACT_TANH = 1, GANMF_ACT_RELU = 2, GANMF_ACT_SIGMOID = 3 };

/* Tensor ids.  Discriminator tensors are numbered in the order of the reference's
 * tf.get_collection(TRAINABLE_VARIABLES, scope) (GANMF.py:121, DisGANMF.py:121):
 *   GANMF:    0 encoding/kernel [N,e]  1 encoding/bias [e]  2 decoding/kernel [e,N]  3 decoding/bias [N]
 *   DisGANMF: 2l layer_l/kernel  2l+1 layer_l/bias (l < d_layers)  2L D_output/kernel [e,1]  2L+1 D_output/bias [1]
 * Generator tensors (GANMF.py:122): */
#define GANMF_T_USER_EMB 100 /* generator/user_embeddings [U,k] */
#define GANMF_T_ITEM_EMB 101 /* generator/item_embeddings [N,k] */
/* CFGAN: the discriminator's ids are DisGANMF's (2l D_hidden_l/kernel -- layer 0 is [2N, e], condition rows first -- 2l+1 its bias,
 * 2L D_output/kernel [e,1], 2L+1 D_output/bias [1]); the generator's start here and are laid out the same way:
 * G0 + 2l G_hidden_l/kernel ([N, g] for l = 0, else [g, g]), G0 + 2l+1 its bias, G0 + 2Lg G_output/kernel [g, N], G0 + 2Lg+1 G_output/bias [N] */
#define GANMF_T_CFGAN_G0 200
/* CAAE: D/disc_user_embeddings and D/disc_item_embeddings are GANMF_T_USER_EMB / GANMF_T_ITEM_EMB, D/disc_item_bias [1, N] is
 * GANMF_T_CAAE_ITEM_BIAS; the layers of G start at GANMF_T_CAAE_G0 and those of G' at GANMF_T_CAAE_GPR0, each laid out as CFGAN's generator:
 * + 2l g_layer_l/kernel ([N, g] for l = 0, else [g, g]), + 2l+1 its bias, + 2Lg g_reconstruction/kernel [g, N], + 2Lg+1 its bias [N] */
#define GANMF_T_CAAE_ITEM_BIAS 102
#define GANMF_T_CAAE_G0 300
#define GANMF_T_CAAE_GPR0 400

/* which copy of a tensor */
enum { GANMF_SLOT_PARAM = 0, GANMF_SLOT_ADAM_M = 1, GANMF_SLOT_ADAM_V = 2, GANMF_SLOT_BEST = 3 };

/* Hyper-parameters = the kwargs of fit() (GANMF.py:88-90, DisGANMF.py:83-85) that enter the graph. */
typedef struct ganmf_cfg {
  int32_t abi_version;      /* GANMF_ABI_VERSION */
  int32_t model;            /* GANMF_MODEL_* */
  int64_t num_users;        /* rows held by THIS handle (a shard when world_size > 1) */
  int64_t num_items;        /* profile width N */
  int32_t num_factors;      /* k */
  int32_t emb_dim;          /* GANMF emb_dim / DisGANMF d_nodes */
  int32_t d_layers;         /* DisGANMF only */
  int32_t d_act;            /* DisGANMF only, GANMF_ACT_* */
  int32_t batch_size;       /* rows per minibatch on this handle */
  float d_lr, g_lr, d_reg, g_reg;
  float m;                  /* GANMF hinge margin multiplier */
  float recon_coefficient;  /* alpha */
  int32_t device;           /* HIP device ordinal */
  int32_t world_size;       /* data-parallel replicas (1 = single GPU) */
  int32_t rank;
  int64_t row_offset;       /* global id of local row 0 (DisGANMF feeds float(uid), DisGANMF.py:110) */
  uint32_t flags;           /* GANMF_FLAG_* */
} ganmf_cfg;

#define GANMF_FLAG_NONE 0u
/* Arithmetic of the GEMM K loops (results are float32 tensors in every case):
 *   default          fp32-accurate: per GEMM either the fp32 MFMA or the bf16 matrix cores with each operand
 *                    split exactly into three bf16 pieces and six piece products accumulated in fp32 (chosen by
 *                    the planner from the grid size; both pass every parity test)
 *   GANMF_FLAG_MFMA_F32   force v_mfma_f32_32x32x2_f32 on the fp32 operands
 *   GANMF_FLAG_MFMA_BF16  operands rounded to ONE bf16 (RNE), fp32 accumulate, fp32 master weights and Adam
 *                    (8 significant bits, fp32's exponent range: no scaling needed).
 *   GANMF_FLAG_MFMA_F16   BASELINE configs[4] as written: operands rounded to ONE IEEE fp16 for
 *                    v_mfma_f32_32x32x16_f16 (same matrix-core rate as bf16, 11 significant bits), fp32 accumulate,
 *                    fp32 master weights and Adam.  Gradient-carrying operands are scaled by a power of two at
 *                    conversion and the sum scaled back in fp32 (static loss scaling per GEMM).
 *   In both low-precision modes DisGANMF's float(uid) input column (DisGANMF.py:59,110-111) does NOT go through
 *   the low-precision K loop: its forward term is added in fp32 in the layer-0 epilogue and its weight-row
 *   gradient is an fp32 reduction of its own. */
#define GANMF_FLAG_MFMA_F32 1u
#define GANMF_FLAG_MFMA_BF16 2u
#define GANMF_FLAG_MFMA_F16 4u

/* Replaces: tf.reset_default_graph + build() + optimizers + Session + initialize_all_variables
 * (GANMF.py:97-105,146-149).  Parameters start at zero; the host uploads initial values with
 * ganmf_set_tensor (the reference's Glorot init happens inside TF and is not reproducible). */
int ganmf_create(const ganmf_cfg* cfg, ganmf_handle** out);
int ganmf_destroy(ganmf_handle* h);

/* Data-parallel setup (no reference counterpart: the reference is single-device).  Rank 0 calls
 * ganmf_comm_unique_id, the host broadcasts the 128 bytes, every rank calls ganmf_comm_init. */
int ganmf_comm_unique_id(uint8_t out128[128]);
int ganmf_comm_init(ganmf_handle* h, const uint8_t id128[128]);
/* What the communicator itself reports (bench.py's `parallelism` object): ranks in the RCCL communicator (ncclCommCount) and this
 * handle's rank in it (ncclCommUserRank); the loopback communicator reports its group.  0 / -1 without a communicator. */
int ganmf_comm_info(ganmf_handle* h, int32_t* world_size, int32_t* rank);
/* In-process alternative to the RCCL communicator: the world_size handles that call this with the same group_id
 * (same process, same device, one host thread each) all-reduce among themselves by rendezvous; sums run in rank
 * order.  For exercising the data-parallel path with world_size > 1 on one GPU (tests/test_gpu_dist_local.py). */
int ganmf_comm_init_local(ganmf_handle* h, int32_t group_id);
/* Ends the handle's communicator WITHOUT touching anything else of the handle: the loopback group is marked failed and its waiting
 * members wake up with an error; an RCCL communicator is aborted (ncclCommAbort).  The one entry point that may be called from
 * another host thread while the handle's own thread is inside a training call -- how a driver whose peer rank failed gets the
 * survivors out of a collective that can no longer complete, BEFORE it destroys their handles (ganmf_amd/dist.py _ThreadRank.kill).
 * Training calls on the handle fail from then on; ganmf_destroy is the only thing left to do with it. */
int ganmf_comm_abort(ganmf_handle* h);

/* Replaces the per-minibatch host work `URM_train[uids].toarray()` + feed_dict upload
 * (GANMF.py:183-187,198-201): the CSR matrix (training orientation, this handle's rows) is
 * uploaded ONCE and minibatch rows are expanded on the device.  Any scipy CSR is accepted, as the reference accepts
 * it: rows whose column indices are unsorted or repeated are made canonical on the host before the upload (columns
 * ascending, the values of a repeated (row, column) summed in stored order, explicit zeros kept -- scipy's
 * sum_duplicates() + sort_indices()), so the device sees what URM_train[uids].toarray() would give. */
int ganmf_set_urm_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices,
                      const float* data, int64_t n_rows, int64_t n_cols);

/* Replaces sess.run(var) / sess.run(var.assign(x)) on one variable (GANMF.py:294-302,
 * Utils_.py:292-294,305-310).  `n` must equal the tensor's element count (row-major, unpadded).
 * Data-parallel handles (communicator attached, world_size > 1): the Adam moments (GANMF_SLOT_ADAM_M / _V) of the
 * REPLICATED tensors (item_embeddings and every discriminator tensor) live sharded over the ranks -- rank r updates
 * slice r only -- so these two slots are rejected (-1) for them; parameters and the best snapshot are whole and identical
 * on every rank, and user_embeddings (rank-owned rows) is whole in every slot.
 * Guarantee (single-GPU handle; tests/test_gpu_warm_start.py): GANMF_SLOT_PARAM + GANMF_SLOT_ADAM_M + GANMF_SLOT_ADAM_V of every
 * tensor id, together with the four powers of ganmf_get_adam_powers, are the COMPLETE training state.  A fresh handle of the same
 * configuration and URM that is given them continues the run they were read from bit for bit (losses, tensors, moments, scores),
 * and writing a handle's own exported state back into it changes nothing: whatever else a handle keeps (the live side of the
 * item_embeddings double buffer, cached operand copies, lr_t tables, per-pass arenas) is derived from them. */
int ganmf_set_tensor(ganmf_handle* h, int tensor_id, int slot, const float* host, int64_t n);
int ganmf_get_tensor(ganmf_handle* h, int tensor_id, int slot, float* host, int64_t n);
int ganmf_tensor_shape(ganmf_handle* h, int tensor_id, int64_t* rows, int64_t* cols);

/* Adam beta-power accumulators of the two optimizers (AdamOptimizer._finish): 4 floats
 * {b1p_D, b2p_D, b1p_G, b2p_G} -- in this order: a discriminator step advances the first pair, a generator step the second;
 * exposed for save/restore and tests.  Part of the complete training state (see ganmf_set_tensor): lr_t of the next step is
 * formed from them, nothing else remembers the step count. */
int ganmf_get_adam_powers(ganmf_handle* h, float out4[4]);
int ganmf_set_adam_powers(ganmf_handle* h, const float in4[4]);

/* Replaces one pass of the `while epoch` body (GANMF.py:175-203): given this epoch's already
 * shuffled row order `perm` (GANMF.py:175; local row ids), runs d_steps passes of discriminator
 * updates over consecutive slices of batch_size rows (ragged tail kept) and then g_steps passes
 * of generator updates over the same slices.  Losses are the pre-update values the reference's
 * sess.run([train, loss]) returns (GANMF.py:186-187,200-201); arrays hold
 * d_steps*ceil(n/batch) resp. g_steps*ceil(n/batch) floats (may be NULL).
 * With world_size > 1 `n_steps_per_pass` (>= ceil(n/batch)) forces every rank to issue the same
 * number of collectives; pass 0 for the default.  `global_batch_rows[i]` = rows in the i-th slice
 * summed over all ranks (NULL when world_size == 1).  Blocking.
 * Because the reference freezes the generator for a whole discriminator pass and the discriminator for a whole
 * generator pass (GANMF.py:176-189, 191-203), the call does per PASS what does not depend on the steps before it --
 * the CSR rows and generated rows of every full minibatch of a discriminator pass; with g_reg == 0 the all-rows
 * Adam over user_embeddings of a generator pass -- with the float operations of the per-step form, bit for bit
 * (GANMF_TUNE=pass_stage=0,lazy_rows=0 runs every step on its own).  Parameters and moments
 * are consistent whenever the call has returned. */
int ganmf_train_epoch(ganmf_handle* h, const int32_t* perm, int64_t n, int32_t d_steps,
                      int32_t g_steps, int64_t n_steps_per_pass, const int32_t* global_batch_rows,
                      float* d_losses, float* g_losses);

/* The same pass with slices of GIVEN sizes: slice i takes the next local_batch_rows[i] rows of `perm`
 * (0 <= local_batch_rows[i] <= batch_size, their sum == n, n_steps_per_pass entries), global_batch_rows[i]
 * (>= local_batch_rows[i], >= 1) as above.  This is how a row-sharded fit() replays the REFERENCE's minibatch
 * schedule (GANMF.py:175-203) on several GPUs: every global minibatch of the single shuffled permutation is
 * split by row owner, so rank r's i-th slice is "the rows of global minibatch i that rank r owns" -- a variable
 * count -- and the union over ranks is exactly the minibatch the reference would have drawn
 * (ganmf_amd/dist.py split_by_owner).  Loss arrays hold d_steps * n_steps_per_pass resp. g_steps * n_steps_per_pass
 * floats.  Blocking. */
int ganmf_train_epoch_ragged(ganmf_handle* h, const int32_t* perm, int64_t n, int32_t d_steps, int32_t g_steps,
                             int64_t n_steps_per_pass, const int32_t* global_batch_rows,
                             const int32_t* local_batch_rows, float* d_losses, float* g_losses);

/* Single updates on an explicit id list (same arithmetic as inside ganmf_train_epoch); used by
 * tests and by callers that schedule batches themselves.  kind: 0 = D-step, 1 = G-step. */
int ganmf_train_step(ganmf_handle* h, int kind, const int32_t* uids, int32_t n, float* loss);

/* Replaces _compute_item_score (GANMF.py:285-292, DisGANMF.py:257-262).
 *   transposed = 0 (user mode): out[i, :] = U[ids[i]] . V^T          -> [n, num_items]
 *   transposed = 1 (item mode): out[i, :] = (U V^T)^T[ids[i]] = V[ids[i]] . U^T -> [n, num_users]
 * (the item-mode product is formed directly; the full matrix is never materialised). */
int ganmf_scores(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, float* out);

/* Replaces the per-user part of BaseRecommender.recommend (Base/BaseRecommender.py:189-234): the scores
 * of ganmf_scores stay on the device, already-seen items are set to -inf and the `cutoff` best items per
 * row are selected there; only n*cutoff ids (and their scores) cross PCIe.  SURVEY §8(f) row 1.
 * ganmf_set_seen_csr uploads URM_train in EVALUATION orientation (rows = users as evaluators see them,
 * columns = items; n_rows/n_cols must match the id domain / score width of the chosen `transposed`).
 * Ties go to the smaller item id; rows with fewer than `cutoff` finite scores are padded with -1.
 * cutoff <= GANMF_RECOMMEND_MAX_CUTOFF (the selection runs `cutoff` arg-max rounds per row; full rankings are
 * the job of ganmf_scores + a host sort). */
#define GANMF_RECOMMEND_MAX_CUTOFF 1024
int ganmf_set_seen_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols);
int ganmf_recommend(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int32_t cutoff, int remove_seen,
                    int32_t* out_items, float* out_scores);

/* The MF contract's two masking rules for everything scored afterwards -- ganmf_scores, ganmf_recommend, ganmf_evaluate
 * (Base/BaseMatrixFactorizationRecommender.py:113-119: `items_to_compute` given -> every OTHER item scores -inf; :128-143: a user
 * without a training interaction ("cold") scores -inf for ALL items; the reference's GANMF._compute_item_score, GANMF.py:285-292,
 * accepts items_to_compute and ignores it).  items == NULL / n_items == 0: no item restriction.  mask_cold_rows != 0: rows that are
 * empty in the matrix of ganmf_set_seen_csr (URM_train, evaluation orientation) are cold; it must be set when the scoring call is
 * made.  The filter stays until it is set again.  A handle starts WITHOUT either mask, which is the reference GANMF's own contract
 * (GANMF.py:285-292: finite scores for every user, items_to_compute ignored); the host classes switch the masks on only under
 * score_contract="mf" (ganmf_amd/GANMF.py). */
int ganmf_set_score_filter(ganmf_handle* h, const int32_t* items, int64_t n_items, int mask_cold_rows);

/* Replaces save_current_model / load_model (GANMF.py:249-255, Utils_.py:292-294): device-side
 * copies of all trainable tensors to / from their `best` twins.  As the reference's load_model restores variables only,
 * ganmf_restore_best overwrites GANMF_SLOT_PARAM only: the Adam moments and the beta powers are left untouched and run on. */
int ganmf_snapshot_best(ganmf_handle* h);
int ganmf_restore_best(ganmf_handle* h);

/* Measurement hooks (bench.py).  ganmf_profile_enable(1) makes every kernel launch of the
 * training step be bracketed by hipEvents on the handle's stream; ganmf_profile_read returns per
 * kernel class the number of launches, total milliseconds and total algorithmic FLOPs / bytes. */
/* GANMF_PROF_MAX: an upper bound of the number of kernel classes, for sizing the caller's array.  It was 48 until the library had 48
 * classes and is 64 since ganmf_pure_svd added eight; ganmf_profile_read returns only the classes that were launched and never
 * writes more than `cap` entries, so a caller compiled against the earlier value cannot be overrun; it loses entries only if more
 * than 48 classes ran in one profile.  No structure or signature changed: GANMF_ABI_VERSION stays.  It is 80 since the ganmf_nmf_*
 * entries added seven, under the same rule. */
#define GANMF_PROF_MAX 80
typedef struct ganmf_prof_entry {
  char name[48];
  int64_t launches;
  double ms;
  double flops;   /* algorithmic */
  double bytes;   /* algorithmic HBM bytes */
} ganmf_prof_entry;
int ganmf_profile_enable(ganmf_handle* h, int on);
/* Device time of a region of calls (bench.py's timed K steps; SURVEY 8(d): hipEvent timing): stop = 0 records a start event on
 * the handle's stream, stop = 1 records the stop event, waits for it and returns the milliseconds between the two -- the time the
 * stream spent on everything enqueued in between, host gaps between blocking calls included, launch latency of the first call
 * excluded.  Nothing in the reference corresponds to it (GANMF.py:172-203 times nothing). */
int ganmf_stream_timer(ganmf_handle* h, int stop, double* ms);
int ganmf_profile_read(ganmf_handle* h, ganmf_prof_entry* out, int32_t cap, int32_t* n_out);

/* Hold-out evaluation on the device (replaces the per-user metric loop of
 * Base/Evaluation/Evaluator.py:262-335 with the definitions of Base/Evaluation/metrics.py): ganmf_evaluate ranks the rows
 * `ids` exactly as ganmf_recommend does (cutoff = the largest of `cutoffs`), looks every recommended item up in the test
 * matrix and returns, per cut-off, the SUMS over the n users of
 *   ROC_AUC, PRECISION, PRECISION_RECALL_MIN_DEN, RECALL, MAP, MRR, NDCG, HIT_RATE, ARHR      (GANMF_EVAL_METRICS values, this order)
 * in float64; only n_cutoffs * 9 doubles cross PCIe.  ganmf_set_test_csr uploads URM_test in EVALUATION orientation with
 * column indices sorted inside each row and `gains` = 2^rating - 1 per stored entry; `disc[k]` = 1 / ln(k + 2) and
 * `ideal_cum[i, k]` = the prefix sums of user i's ideal DCG terms (both [.., max cutoff], formed by the caller the way
 * the reference forms them, in float32 where it does).  At most GANMF_EVAL_MAX_CUTOFFS cut-offs per call. */
#define GANMF_EVAL_METRICS 9
#define GANMF_EVAL_MAX_CUTOFFS 8
int ganmf_set_test_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const double* gains, int64_t n_rows,
                       int64_t n_cols);
int ganmf_evaluate(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, const int32_t* cutoffs,
                   int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums);

/* The reference's full metric row on the device (Base/Evaluation/Evaluator.py:262-335 with every metric object that
 * create_empty_metrics_dict builds, Evaluator.py:43-84; DIVERSITY_SIMILARITY, which the reference adds only for a diversity_object,
 * comes from ganmf_evaluate_diversity below, ignore_items from ganmf_set_items_to_ignore; ignore_users is the caller's id list).
 * ganmf_set_test_ratings: the rating (float32) of every stored entry of the matrix ganmf_set_test_csr holds, in its order;
 *   each ganmf_set_test_csr drops them.  Needed by RMSE (metrics.py:634 rmse).
 * ganmf_set_eval_item_weights: two per-item vectors of the evaluation width, formed by the caller in float64 from the
 *   per-column nnz `pop` of URM_train (evaluation orientation, zeros eliminated; Evaluator.py:250):
 *   novelty[i] = -log2(pop[i] / sum(pop)) / len(pop), 0 where pop[i] = 0 (metrics.py:298-347 Novelty),
 *   popularity[i] = pop[i] / max(pop) (metrics.py:355-398 AveragePopularity).  The device only gathers and adds them.
 * ganmf_evaluate_full: ganmf_evaluate's ranking and lookups, and in the same selection kernel -- after the seen mask and the
 *   score filter, before the first selection round -- each row's fp32 RMSE over its test items (NaN when no error is finite).
 *   sums[n_cutoffs, GANMF_EVAL_FULL_METRICS] (overwritten): ganmf_evaluate's nine sums, then the sums over the n users of
 *     RMSE, NOVELTY (novelty summed over the list cut at c), AVERAGE_POPULARITY (mean popularity of a non-empty list, else 0)
 *     and the number of non-empty lists (Coverage_User).
 *   counts[n_cutoffs, W] (ADDED into): times each item appears in the lists cut at each cut-off -- what Coverage_Item,
 *     Gini_Diversity, Shannon_Entropy, Diversity_Herfindahl and Diversity_MeanInterList count (metrics.py:30-280,465-551);
 *     the host finishes those from the counts summed over all its calls.
 *   Same limits as ganmf_evaluate; also needs both uploads above for the current test matrix and width. */
#define GANMF_EVAL_FULL_METRICS 13
int ganmf_set_test_ratings(ganmf_handle* h, const float* ratings, int64_t nnz);
int ganmf_set_eval_item_weights(ganmf_handle* h, const double* novelty, const double* popularity, int64_t width);
int ganmf_evaluate_full(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, const int32_t* cutoffs,
                        int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums, int64_t* counts);

/* Negative-sample evaluation on the device (Base/Evaluation/Evaluator.py:419-590, EvaluatorNegativeItemSample): every user's test
 * items are ranked only against that user's own candidate list, URM_test + URM_test_negative.  The reference forms a full-width score
 * row per user and masks it down to the candidates; these entries gather the factor rows of the candidates and form only those dot
 * products (ganmf_amd/csrc/cand_topk.hpp), so the [n, W] score matrix never exists.  They always restrict to the candidates -- the MF
 * contract's items_to_compute rule (Base/BaseMatrixFactorizationRecommender.py:113-119), whatever score filter is set; the filter of
 * ganmf_set_score_filter (item list, cold rows) applies on top of it.
 * ganmf_set_candidates_csr: replaces URM_items_to_rank and _get_user_specific_items_to_compute (Evaluator.py:450-463).  The matrix
 *   is in EVALUATION orientation like ganmf_set_seen_csr (n_rows / n_cols must match the id domain / score width of the `transposed`
 *   it is used with); stored entries are the candidates, values do not matter.  Any CSR is accepted: rows are sorted and a repeated
 *   column is kept once on the host before the upload (the reference's sum of two boolean matrices de-duplicates the same way).
 *   indptr == NULL drops the held matrix.
 * ganmf_recommend_candidates: replaces the per-user recommend(user, items_to_compute = candidates) call and the ranking inside it
 *   (Evaluator.py:504-513, 527).  Arguments, outputs, tie rule (smaller item id) and -1 / -inf padding as ganmf_recommend; a row with
 *   fewer than `cutoff` unmasked candidates is padded.  Scores are fp32 sums in a fixed order: the same bytes on every call and handle.
 * ganmf_evaluate_candidates: replaces the metric loop Evaluator.py:496-564 (sums; the host divides as :586-599 does).  The ranking of
 *   ganmf_recommend_candidates at the largest cut-off, then ganmf_evaluate's metric kernel (counts == NULL: sums[n_cutoffs, 9]) or
 *   ganmf_evaluate_full's (counts != NULL: sums[n_cutoffs, 13] overwritten, counts[n_cutoffs, W] added into; needs
 *   ganmf_set_test_ratings and ganmf_set_eval_item_weights like it; RMSE (Evaluator.py:528) over the test items that are candidates
 *   with a finite score).  Same cut-off limits as those two calls.
 * A row may hold at most GANMF_CANDIDATES_MAX_PER_ROW candidates (one workgroup's LDS holds a row's scores and ids).  Errors (-1, message
 *   in ganmf_last_error, nothing enqueued, the handle usable as before): no candidate matrix set, its shape does not match
 *   `transposed`, a requested row over the limit, and the argument errors of ganmf_recommend / ganmf_evaluate(_full). */
#define GANMF_CANDIDATES_MAX_PER_ROW 8192
int ganmf_set_candidates_csr(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols);
int ganmf_recommend_candidates(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int32_t cutoff, int remove_seen,
                               int32_t* out_items, float* out_scores);
int ganmf_evaluate_candidates(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, const int32_t* cutoffs,
                              int32_t n_cutoffs, const double* disc, const double* ideal_cum, double* sums, int64_t* counts);

/* Hold-out metrics per user and per group of users on the device -- what the reference's user-activity study computes in a Python loop
 * over a [users, items] score matrix (MFLearned.py:80-145: MAP@20 of every user, averaged per bucket of interaction counts), and what
 * metrics per segment / fold or a significance test over users need.
 * ganmf_evaluate_groups ranks the rows `ids` exactly as ganmf_evaluate does (candidates = 0: the full width, with the score filter and
 *   the seen mask as set) or as ganmf_evaluate_candidates does (candidates = 1: each row among its own candidates); test matrix, `disc`,
 *   `ideal_cum`, cut-off limits and tie rule are those calls'.  The per-user values are the ones those calls sum (one device function
 *   forms them for all three).
 *   group_of[i] in [-1, n_groups): the group of position i of `ids`; -1: ranked and written to per_user, counted in no group.
 *   group_sums[n_groups, n_cutoffs, GANMF_EVAL_METRICS] (overwritten): the sums of the nine values over each group's members, float64,
 *     added in a fixed order without floating-point atomics -- the same bytes on every call and handle.  group_size[n_groups]: the
 *     member counts.  An empty group gets zeros.  0 <= n_groups <= GANMF_EVAL_MAX_GROUPS.
 *   per_user: NULL, or [n, n_cutoffs, GANMF_EVAL_METRICS] float64 in position order.
 *   group_of == NULL with n_groups == 0 is allowed when per_user != NULL (per-user values only).
 * Only group_sums, group_size and per_user (if asked for) cross PCIe; the [n, W] score matrix never does.  Parameters, Adam state, the
 * score filter and the held test / candidate / seen matrices are not modified.  Errors (-1, message in ganmf_last_error, nothing
 * enqueued, the handle usable as before): every argument error of ganmf_evaluate / ganmf_evaluate_candidates, n_groups out of range,
 * a group_of entry out of range, and a call that asks for neither groups nor per_user. */
#define GANMF_EVAL_MAX_GROUPS 256
int ganmf_evaluate_groups(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, int candidates,
                          const int32_t* cutoffs, int32_t n_cutoffs, const double* disc, const double* ideal_cum,
                          const int32_t* group_of, int32_t n_groups, double* group_sums, int64_t* group_size, double* per_user);

/* The evaluators' ignore_items and the recommender's remove_CustomItems_flag / remove_top_pop_flag on the device
 * (Base/BaseRecommender.py:72-90, 207-211: scores_batch[:, items] = -inf after the seen mask, before the top-k; Evaluator.py:369-370,
 * 410-411: set around a whole evaluation).
 * ganmf_set_items_to_ignore: handle state like the score filter, a byte mask (a repeated id is harmless); items == NULL or
 *   n_items == 0 clears it.  While set, the listed columns score -inf in everything that RANKS, under both score contracts and in
 *   addition to the filter of ganmf_set_score_filter: ganmf_recommend, ganmf_recommend_candidates, ganmf_evaluate, ganmf_evaluate_full,
 *   ganmf_evaluate_candidates, ganmf_evaluate_groups and ganmf_evaluate_diversity.  It is applied where the score filter is: before the
 *   RMSE read of the 13-sum evaluations (an ignored test item does not count in RMSE, as in the reference, whose masked score matrix
 *   is what return_scores hands to rmse) and before the first selection round.  It does NOT apply to ganmf_scores,
 *   ganmf_score_similarity or training (_compute_item_score is not affected in the reference either).  Range checks as
 *   ganmf_set_score_filter: against max(num_users, num_items) here, against the score width in use when a ranking entry runs (-1).
 *
 * Intra-list diversity of the ranked lists (Base/Evaluation/metrics.py:405-452 Diversity_similarity; the reference's
 * DIVERSITY_SIMILARITY, present only when the evaluator was given a diversity_object, Evaluator.py:83-85).
 * ganmf_set_item_diversity: `matrix` is [width, width] row-major float32 (the caller rounds a float64 matrix once and uses the
 *   rounded values on every route), resident until replaced; NULL drops it.  A matrix over a quarter of the free device memory is
 *   refused (-1; the rule of ganmf_score_similarity).
 * ganmf_evaluate_diversity ranks the rows `ids` exactly as ganmf_evaluate (candidates = 0) or ganmf_evaluate_candidates
 *   (candidates = 1) does at the largest cut-off -- limits, tie rule, score filter, seen mask and ignore list are those calls' -- and
 *   forms, for every row and cut-off c, with len = the valid ids of the row's list and L_c = min(c, len):
 *     value = sum of D[l_i, l_j] over the ordered pairs i != j with max(i + 2, j + 1) <= L_c, divided by L_c (L_c - 1)
 *   -- the reference's sum: rows i = 0 .. L_c - 2 only (the LAST item's row is never visited; D need not be symmetric), all other
 *   columns.  The value is 0 when L_c < 2 (the reference raises ZeroDivisionError there); the row still counts in the caller's mean.
 *   sums[n_cutoffs] (overwritten): the sums of the values over the n rows; per_user: NULL or [n, n_cutoffs] in position order.
 *   float64 throughout, fixed summation order, no floating-point atomics: the same bytes on every call and handle
 *   (ganmf_amd/csrc/list_diversity.hpp; O(n K^2) gathers for largest cut-off K).
 *   Errors (-1, message in ganmf_last_error, nothing enqueued, the handle usable as before): no matrix held, a held width other than
 *   the score width of `transposed`, NULL ids / cutoffs / sums, n_cutoffs outside [1, GANMF_EVAL_MAX_CUTOFFS], and the argument
 *   errors of ganmf_recommend / ganmf_recommend_candidates. */
int ganmf_set_items_to_ignore(ganmf_handle* h, const int32_t* items, int64_t n_items);
int ganmf_set_item_diversity(ganmf_handle* h, const float* matrix, int64_t width);
int ganmf_evaluate_diversity(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int remove_seen, int candidates,
                             const int32_t* cutoffs, int32_t n_cutoffs, double* sums, double* per_user);

/* Cosine similarity of the predictions on the device: the computation under the reference's collapse study
 * (AblationStudy.py:88-92,113-117: cosine_similarity of all predictions, np.mean and np.std of the [users, users] matrix, and the
 * matrix behind the heat-map).  For the requested rows ids[0..n) (transposed as in ganmf_scores):
 *   s_i = the UNFILTERED score row i of ganmf_scores; s^_i = s_i / ||s_i||_2; c_ij = s^_i . s^_j for all n^2 ordered pairs.
 *   Zero-row rule: a row of norm 0 stays all-zero (sklearn's normalize divides it by 1), so its similarity with every row, itself
 *   included, is 0; such rows are counted in sums[2] and are part of the statistics, as in np.mean / np.std of the sklearn matrix.
 *   No-filter rule: the filter of ganmf_set_score_filter is NOT applied, under either score contract -- a -inf has no cosine, and
 *   the reference's GANMF has no filter.  The filter stays set for the calls that follow.
 * sums = { sum d, sum d^2, number of zero rows, n } with d = c - 1 over the n^2 pairs, in float64: the caller forms
 *   mean = 1 + sums[0] / n^2 and std = sqrt(sums[1] / n^2 - (sums[0] / n^2)^2), the population standard deviation of np.std.  (d is
 *   summed instead of c because the statistic of interest is a collapsed model's, c ~ 1, where this form has no cancellation.)
 * matrix != NULL: receives the [n, n] float32 similarities.  pooled != NULL: receives [pool, pool] block means of that matrix, row
 *   i in bin floor(i * pool / n), 1 <= pool <= min(n, 1024) -- what a figure needs, instead of n^2 values over PCIe.  Both NULL:
 *   statistics only, the matrix is never stored (`pool` is then ignored).
 * The scores stay on the device; the symmetric product forms only the upper triangle of 128 x 128 tiles in fp32-accurate arithmetic
 * (ganmf_amd/csrc/gram_stats.hpp), every sum runs in a fixed order without atomics: the same bytes on every call and handle.
 * Parameters, Adam state and the score filter are not touched.  Errors (-1, message in ganmf_last_error, nothing enqueued, the
 * handle usable as before): null ids / sums, n < 1, an id out of range, a bad pool, and a call whose buffers would take more than
 * a quarter of the free device memory. */
int ganmf_score_similarity(ganmf_handle* h, const int32_t* ids, int64_t n, int transposed, int32_t pool, double sums[4], float* pooled,
                           float* matrix);

/* Discriminator inference on the device: the discriminator's view of a profile, for stored rows and for generated ones.  Replaces the
 * reference's autoencoder_codes() (GANMF.py:304-307: encoding of the whole densified training matrix) and exposes, per row, the two
 * terms its discriminator losses average over a batch (GANMF.py:62-70; DisGANMF.py:57-65).
 * `rows` are generator rows in training orientation (in item mode: catalogue items): they index the matrix of ganmf_set_urm_csr and
 * the rows of user_embeddings.  generated = 0: the input x is the stored CSR row (never densified on the host; GANMF reads it as CSR
 * on the device as well).  generated = 1: x = U[rows] . V^T, unfiltered -- neither the score filter nor the ignore list applies.
 *   GANMF:     features [n, emb_dim] = E = x . We + be;   value [n] = the EBGAN energy D(x) = sum_j (dec(E)_j - x_j)^2 / num_items
 *              (tf.losses.mean_squared_error of GANMF.py:68 taken per row).  The reconstruction is never stored.
 *   DisGANMF:  features [n, d_nodes] = the output of the last hidden layer (what feature matching compares, DisGANMF.py:132-136);
 *              value [n] = the logit.  The float(uid) input is row_offset + rows[i].
 * Either output may be NULL (not computed where that saves work), not both.  n = 0 returns 0 and writes nothing.
 * Every product runs in the fp32-accurate arithmetic (exact three-way bf16 split or fp32 MFMA), also on a handle created with
 * GANMF_FLAG_MFMA_BF16 / _F16: a diagnostic does not carry the training mode's rounding.  Sums run in a fixed order without
 * floating-point atomics: the same bytes on every call and handle.  The rows are processed in blocks whose buffers -- the call's own --
 * stay under a quarter of the free device memory; ganmf_set_discriminate_block caps the rows per block (0: that rule alone).
 * Parameters, Adam moments, the beta powers and every per-pass state of training are not modified.
 * Errors (-1, message in ganmf_last_error, nothing enqueued, the handle usable as before): a row outside [0, num_users), stored rows
 * asked for before ganmf_set_urm_csr, both outputs NULL, n < 0. */
int ganmf_set_discriminate_block(ganmf_handle* h, int64_t rows);
int ganmf_discriminate(ganmf_handle* h, const int32_t* rows, int64_t n, int generated, float* features, double* value);

/* Implicit-feedback ALS (WRMF) on the device: replaces the per-row Python loop of the reference's IALS
 * (MatrixFactorization/IALSRecommender.py:137-201, _run_epoch / _update_row: one np.linalg.inv per user and per item per epoch).  The
 * entries act on the tensors GANMF_T_USER_EMB / GANMF_T_ITEM_EMB of ANY single-GPU handle; a GANMF_MODEL_MF handle has nothing else.
 * ganmf_als_set_confidence: uploads the handle's weighted sparse matrix, both orientations (ganmf_pure_svd reads the same two uploads,
 *   with the URM's data as the values); for ALS it replaces the confidence matrix C and its transpose (IALSRecommender.py:100-126, _build_confidence_matrix,
 *   C_csc).  side 0: users x items, [num_users, num_items]; side 1: its transpose, [num_items, num_users], which the caller forms.
 *   `conf` holds the confidence c (1 + alpha r, or 1 + alpha log(1 + r / epsilon)) of every stored entry; entries that are not stored
 *   have c = 1 and preference 0.  Any CSR whose columns are in range; a row's entries are summed in stored order.  Resident until
 *   replaced.
 * ganmf_als_half_sweep: one side of _run_epoch.  side 0 rewrites the user factors X from the item factors Y (IALSRecommender.py:141-145),
 *   side 1 the item factors from the user factors (:147-151).  For every row u with at least one stored entry, with P(u) its columns,
 *     B = Y^T Y + sum_{j in P(u)} (c_j - 1) y_j y_j^T + reg I,   b = sum_{j in P(u)} c_j y_j,   X[u, :] = B^-1 b        (:167-201)
 *   Rows without a stored entry are not touched (the reference loops over warm rows only, :139-140).  Y^T Y is one fp32-MFMA product
 *   per call; the rows are solved by als_rows_kernel (ganmf_amd/csrc/als_rows.hpp): fp32 throughout, Cholesky instead of the reference's
 *   inverse, no atomics, fixed summation order -- the same bytes on every call and handle.  Blocking.
 *   Errors: -1 with nothing enqueued for num_factors > GANMF_ALS_MAX_FACTORS (a row's packed triangle has to fit the 160 KiB of LDS of a
 *   CU), a side without confidences, a data-parallel handle; -4 when a row's system is not positive definite in fp32 (reg <= 0 with
 *   rank-deficient factors, or a reg below the rounding of Y^T Y, about 1e-7 of its largest entry, with such factors): the message names the first such row, those rows keep their factors, all others are updated. */
#define GANMF_ALS_MAX_FACTORS 256
int ganmf_als_set_confidence(ganmf_handle* h, int side, const int64_t* indptr, const int32_t* indices, const float* conf, int64_t n_rows,
                             int64_t n_cols);
int ganmf_als_half_sweep(ganmf_handle* h, int side, float reg);

/* PureSVD on the device: replaces sklearn.utils.extmath.randomized_svd as the reference's PureSVDRecommender calls it
 * (MatrixFactorization/PureSVDRecommender.py:29-37: n_components = num_factors, defaults otherwise).  Acts on GANMF_T_USER_EMB /
 * GANMF_T_ITEM_EMB of ANY single-GPU handle, a GANMF_MODEL_MF one included.  The two uploads of ganmf_als_set_confidence are "the
 * handle's weighted sparse matrix, both orientations": for the ALS entries the values are confidences, for this entry they are the
 * URM's data (side 0 the URM, side 1 its transpose).
 *   omega: host array [min(num_users, num_items), n_random], row-major: the random test matrix (the caller draws it, so a seeded run
 *   equals the reference's); n_random = num_factors + oversampling (sklearn: + 10); n_iter power iterations (sklearn: 7 if
 *   num_factors < 0.1 min(shape), else 4).  With M = URM if num_users >= num_items, else URM^T:
 *     Q = omega;  n_iter times: Q = orth(M Q), Q = orth(M^T Q);  Q = orth(M Q);  Z = M^T Q;  Z^T Z = W diag(lambda) W^T (descending)
 *     left = Q W[:, :k],  sigma . right = Z W[:, :k],  sigma = the column norms of Z W[:, :k]
 *   USER = left, ITEM = Z W (M = URM), or USER = Z W / sigma, ITEM = (Q W) sigma (M = URM^T); every column of USER has its entry of
 *   largest magnitude positive, ITEM's column carries the same sign (sklearn's svd_flip).  orth is Cholesky-QR applied twice
 *   (sklearn normalises by LU between power iterations: with the same omega the result is the same subspace); the eigenpairs come
 *   from a one-sided Jacobi iteration (ganmf_amd/csrc/svd_rows.hpp).  fp32 throughout, no atomics, fixed summation order: the same
 *   bytes on every call.  sigma (may be NULL) receives the num_factors singular values.  Blocking.  Pad columns stay zero.
 *   Errors: -1 with nothing enqueued for n_random < num_factors, n_random > min(num_users, num_items), n_random >
 *   GANMF_SVD_MAX_RANDOM (the Cholesky factor's packed triangle has to fit the 160 KiB of LDS of a CU), n_iter < 0, a value of omega
 *   that is not finite, a side that has not been uploaded, a data-parallel handle.  -4 when a Cholesky factorisation meets a pivot
 *   that is not positive (the matrix has a rank below n_random, or Cholesky-QR lost it in fp32), when the eigensolver has not
 *   converged after 30 sweeps, or when one of the num_factors eigenvalues kept is not positive: the message names the stage (which
 *   half step, which pass).  The factor tensors are written only after all of this has been checked: any failure leaves them as
 *   they were. */
#define GANMF_SVD_MAX_RANDOM 280
int ganmf_pure_svd(ganmf_handle* h, const float* omega, int n_random, int n_iter, float* sigma);

/* NMF on the device: the two solvers of sklearn.decomposition.NMF as the reference's NMFRecommender runs them
 * (MatrixFactorization/NMFRecommender.py:65-78: alpha_W = alpha_H = 0, so no regularisation term; float32).  The entries act on
 * W = GANMF_T_USER_EMB [num_users, k] and H^T = GANMF_T_ITEM_EMB [num_items, k] of ANY single-GPU handle, a GANMF_MODEL_MF one
 * included, as the caller set them (ganmf_set_tensor: the initial factors are the caller's, like every random number), and read X
 * from the two uploads of ganmf_als_set_confidence (side 0 the URM, side 1 its transpose, the URM's data as the values).  The host
 * decides when to stop: every entry runs the number of iterations it is given.  EPS = 2^-23.
 * ganmf_nmf_mu: n_iter iterations of the multiplicative update (sklearn's _fit_multiplicative_update, gamma = 1).
 *   GANMF_NMF_FROBENIUS: W *= (X H^T) / (W (H H^T)); H *= (W^T X) / ((W^T W) H); a denominator of exactly 0 becomes EPS.
 *   GANMF_NMF_KULLBACK_LEIBLER: with q_ij = x_ij / max(w_i . h_j, EPS) at the stored entries, W *= (Q H^T) / rowsum(H) (0 -> EPS); Q
 *   again from the new W; H *= (W^T Q) / colsum(W) (0 -> 1); entries of H below 2^-52 become 0.
 *   update_H = 0 runs the W half only (sklearn's transform): X H^T, H H^T and rowsum(H) are then formed once per call.
 *   error (may be NULL) receives ganmf_nmf_error of the factors after the last iteration.
 * ganmf_nmf_cd: n_iter iterations of coordinate descent on the Frobenius loss (sklearn's _update_cdnmf_fast): a W half, then with
 *   update_H an H half, the same routine on X^T, H^T, W.  A half forms G = H H^T and B = X H^T and, for every row i and every t in the
 *   order of its permutation: grad = G[t, :] . W[i, :] - B[i, t]; the violation grows by |min(0, grad)| if W[i, t] == 0, else by |grad|;
 *   W[i, t] = max(W[i, t] - grad / G[t, t], 0) if G[t, t] != 0.  perms: host array [n_iter, update_H ? 2 : 1, k], one permutation of
 *   0 .. k - 1 per half in the order the halves run; violation [n_iter] receives every iteration's sum over its halves (float64).
 * ganmf_nmf_error: sklearn's _beta_divergence(X, W, H, beta_loss, square_root=True) of the factors as they stand:
 *   sqrt(max(|X|^2 + tr((W^T W)(H H^T)) - 2 tr((X H^T) W^T), 0)), or sqrt(2 max(r, 0)) with r = sum_{x > EPS} x log(x / max(wh, EPS)) +
 *   colsum(W) . rowsum(H) - sum_{x > EPS} x; every scalar is accumulated in float64.
 * The sparse products are ganmf_pure_svd's kernel, the Gram matrices its fp32 MFMA product; the row solvers, the sampled products and
 * the reductions are ganmf_amd/csrc/nmf_rows.hpp.  No atomics, fixed summation order: the same bytes on every call.  Blocking.  Pad
 * columns stay zero.
 *   Errors: -1 with nothing enqueued for num_factors > GANMF_NMF_MAX_FACTORS, a side that has not been uploaded, sides with different
 *   numbers of stored entries, a data-parallel handle, an unknown beta_loss, n_iter < 0, a row of perms that is not a permutation. */
#define GANMF_NMF_MAX_FACTORS 270
#define GANMF_NMF_FROBENIUS 0
#define GANMF_NMF_KULLBACK_LEIBLER 1
int ganmf_nmf_mu(ganmf_handle* h, int beta_loss, int n_iter, int update_H, double* error);
int ganmf_nmf_cd(ganmf_handle* h, const int32_t* perms, int n_iter, int update_H, double* violation);
int ganmf_nmf_error(ganmf_handle* h, int beta_loss, double* error);

/* Item-based nearest neighbours on the device (KNN/ItemKNNCFRecommender.py; Base/Similarity/Compute_Similarity_Python.py:209-384,
 * which the reference runs in pure Python when its Cython extension is absent).  All three entries need a GANMF_MODEL_ITEMSIM handle.
 * The weighted URM goes up through ganmf_als_set_confidence -- side 0: users x items, side 1: its transpose (the URM by item column)
 * -- in canonical form: inside a row the indices ascend without repeats.
 * ganmf_itemknn_fit: for every item i
 *     w_j = sum_u x_ui x_uj for every item j;  w_i = 0;  the kind's value v_j (below);  the min(topk, num_items) largest v_j are
 *     selected and those that are not zero are kept (Compute_Similarity_Python.py:297-356),
 *   with s = shrink + 1e-6 and the per-item float32 vectors den_a / den_b the caller forms in float64 (the column norms, sums of
 *   squares or their powers, Compute_Similarity_Python.py:242-250):
 *     GANMF_ITEMKNN_PRODUCT      w / (den_a[i] den_b[j] + s)                                    cosine, asymmetric cosine
 *     GANMF_ITEMKNN_TANIMOTO     w / (den_a[i] + den_a[j] - w + s)                              jaccard / tanimoto
 *     GANMF_ITEMKNN_DICE         w / (den_a[i] + den_a[j] + s)
 *     GANMF_ITEMKNN_TVERSKY      w / (w + (den_a[i] - w) p0 + (den_a[j] - w) p1 + s)
 *     GANMF_ITEMKNN_SHRINK_ONLY  w / shrink                                                     not normalised, shrink != 0
 *     GANMF_ITEMKNN_RAW          w
 *   (den_a / den_b may be NULL for the kinds that do not read them; p0 / p1 are read by TVERSKY only).  Every w_j is one fp32 FMA chain
 *   over ascending users, there is no floating-point atomic anywhere: two fits from the same uploads return the same bytes.  Among
 *   exactly equal values the smaller item id is selected: select_topk_nonzero (ganmf_amd/csrc/topk_rounds.hpp), the one selection of
 *   every fit on such a handle, built on the arg-max round of ganmf_recommend.  The [num_items, num_items] matrix of the w_j
 *   never exists: one row per workgroup, in LDS or (wide catalogues) in a private global row.  Any num_items and num_users.  The
 *   handle then holds W BY TARGET ITEM: column i of the reference's W_sparse = the kept neighbours j of item i with their values,
 *   neighbours ascending.  *nnz receives the number of stored entries.  Blocking.
 *   Errors (-1, nothing enqueued, the held W dropped only once every check has passed): an unknown kind, topk < 1 or above
 *   GANMF_ITEMKNN_MAX_TOPK (the selection runs topk arg-max rounds per item; the reference's search space ends at 1000), shrink < 0
 *   or not finite, SHRINK_ONLY with shrink = 0, a missing den vector or a term that is not finite, a side that has not been uploaded
 *   or is not canonical, a data-parallel handle, a handle of another model.
 * ganmf_itemknn_get: the held W to the caller: indptr [num_items + 1], indices / data [nnz] (neighbour ids and weights of every
 *   target item in turn).
 * ganmf_set_item_similarity: uploads a W by target item (a saved model; any other W_sparse model, such as P3alpha or SLIM): row i
 *   of the CSR arrays = column i of W_sparse.  Columns may have any length and order; checks as the other CSR uploads (monotone
 *   indptr from 0, indices in [0, n_items)), n_items must be the handle's num_items, weights finite.
 * Scores on such a handle: out[r, i] = sum over the stored neighbours j of item i of x[ids[r], j] W[j, i], an fp32 FMA chain in stored
 *   order, 0 where nothing is stored (a user without interactions scores 0 everywhere, as in the reference); x is side 0.  The
 *   product is sparse: a workgroup keeps the dense profiles of a group of users in LDS and reads every stored weight once per group.
 *   transposed = 1 is an error (-1). */
#define GANMF_ITEMKNN_MAX_TOPK 1024
enum { GANMF_ITEMKNN_PRODUCT = 0, GANMF_ITEMKNN_TANIMOTO = 1, GANMF_ITEMKNN_DICE = 2, GANMF_ITEMKNN_TVERSKY = 3,
       GANMF_ITEMKNN_SHRINK_ONLY = 4, GANMF_ITEMKNN_RAW = 5 };
int ganmf_itemknn_fit(ganmf_handle* h, int kind, int32_t topk, float shrink, float p0, float p1, const float* den_a, const float* den_b,
                      int64_t* nnz);
int ganmf_itemknn_get(ganmf_handle* h, int64_t* indptr, int32_t* indices, float* data);
int ganmf_set_item_similarity(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_items);

/* User-based nearest neighbours on the device (KNN/UserKNNCFRecommender.py; Base/BaseSimilarityMatrixRecommender.py:95-117: scores =
 * W_sparse[users] . URM_train).  All three entries need a GANMF_MODEL_ITEMSIM handle.  Such a handle holds at most ONE similarity
 * matrix and records whether it is item x item (above) or user x user; every fit and upload, of either kind, drops the held one.
 * ganmf_userknn_fit: ganmf_itemknn_fit with the two sides of the URM exchanged -- for every user i, w_j = sum over the items of
 *   x_i. x_j. for every user j, w_i = 0, the kind's value, the min(topk, num_users) largest kept where not zero -- with the same kinds,
 *   the same selection (ties to the smaller user id) and the same kernel, which reads side 0 (users x items, canonical) in place of
 *   side 1; side 1 is not read.  den_a / den_b are per USER, [num_users] (the row norms, row counts or their powers).  The by-target
 *   result (column i of the reference's W_sparse = the kept neighbours of user i) is then turned into rows INSIDE the call, on the
 *   host: read back, a stable counting sort by the stored neighbour (columns visited in ascending order, so every row ascends),
 *   uploaded -- at most num_users * topk entries; the reference does the same conversion in scipy.  The handle then holds W BY ROW:
 *   row u = the users v with W_sparse[u, v] stored, ascending.  A row is NOT bounded by topk: a user who is in many top-k lists has a
 *   long row.  *nnz receives the number of stored entries.  Blocking.  Same bytes on every call.
 *   Errors as ganmf_itemknn_fit's (-1, nothing enqueued, the held matrix dropped only once every check has passed), with side 0 the
 *   one side that must be uploaded and canonical.
 * ganmf_userknn_get: the held W to the caller as CSR by row: indptr [num_users + 1], indices / data [nnz].  An error (-1) while the
 *   handle holds an item matrix; ganmf_itemknn_get is an error while it holds a user matrix.
 * ganmf_set_user_similarity: uploads W_sparse [n_users, n_users] as CSR by row (a saved model); checks as ganmf_set_item_similarity:
 *   monotone indptr from 0, indices in [0, n_users), n_users the handle's num_users, weights finite.  The chain below runs in stored
 *   order: upload rows with ascending indices for scores that equal a fitted model's.
 * Scores while a user matrix is held: out[r, i] = sum over the stored v of row ids[r] of W[ids[r], v] x[v, i], x side 0: for every
 *   item ONE fp32 FMA chain over the neighbours in stored order that starts at 0; exactly 0 for an item no neighbour rated (and for a
 *   user without neighbours).  No floating-point atomics; a user's scores depend on that user's row of W and on x alone, not on the
 *   batch or the user's place in it.  One workgroup per scored row keeps the row's accumulator in LDS (catalogues up to 32 768 items;
 *   wider ones accumulate in the row of the output itself), each wave owning a contiguous range of items.  Seen mask, score filter,
 *   top-k and every evaluation entry run on these scores unchanged.  transposed = 1 is an error (-1). */
int ganmf_userknn_fit(ganmf_handle* h, int kind, int32_t topk, float shrink, float p0, float p1, const float* den_a, const float* den_b,
                      int64_t* nnz);
int ganmf_userknn_get(ganmf_handle* h, int64_t* indptr, int32_t* indices, float* data);
int ganmf_set_user_similarity(ganmf_handle* h, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_users);

/* The graph-based item models P3alpha and RP3beta on the device (GraphBased/P3alphaRecommender.py:52-141, RP3betaRecommender.py:
 * 49-151): a three-step random walk item -> user -> item, W = Piu^alpha . Pui^alpha with Pui the URM with every user row divided by
 * its L1 norm and Piu ones at the stored entries of the URM's transpose, every item row divided by its stored count deg_i.  Needs a
 * GANMF_MODEL_ITEMSIM handle with both sides uploaded through ganmf_als_set_confidence in canonical form: side 0 is the matrix the
 * scores are formed from; side 1 holds, for this call, Pui^alpha BY ITEM (items x users, the URM's pattern with the transition weights
 * as values, formed by the caller in float64 and rounded once).  Piu^alpha has one value per item, row_scale[i] = (1 / deg_i)^alpha at
 * every user stored in row i of side 1 (a stored explicit zero counts in deg_i and contributes 0 to the product).
 * ganmf_p3_fit:
 *   row pass, for every source item i:
 *     w_j = sum_u row_scale[i] * Pui^alpha[u, j] over the users u stored in row i of side 1, for every item j;
 *     w_j *= col_scale[j] when col_scale is given (RP3beta: deg_j^-beta, 0 where deg_j = 0; NULL for P3alpha);  w_i = 0;
 *     the min(topk, num_items) largest w_j are selected and those that are not zero are kept: row i of R.
 *   normalize != 0: every row of R is divided by the sum of the absolute values of its entries (summed in stored order, ascending
 *     target id, in fp64; one rounding per value).  Empty rows stay empty.
 *   column pass, for every target item j: the min(col_topk, num_items) largest non-zero entries of column j of R are kept (the
 *     reference's similarityMatrixTopK works column-wise).  This pass does no arithmetic: its values are bit copies of R's.
 *     col_topk = 0 skips the selection: R itself, transposed to the handle's layout, is held.
 *   Every w_j is one fp32 FMA chain fmaf(row_scale[i], Pui^alpha[u, j], acc) over ascending users, there is no floating-point atomic
 *   anywhere: two fits from the same uploads return the same bytes.  Among exactly equal values the smaller item id is selected in
 *   both selections (select_topk_nonzero, as in ganmf_itemknn_fit).  One row (column) of the walk per workgroup, in LDS or (wide
 *   catalogues) in a private global row; any num_items and num_users.  The handle then holds W BY TARGET ITEM as after
 *   ganmf_itemknn_fit -- scores[u, j] = sum_i x[u, i] W[i, j], the target is column j, its neighbours are the source rows i, ascending
 *   -- and ganmf_itemknn_get, ganmf_set_item_similarity, the scores and every ranking and evaluation entry work on it unchanged.
 *   *nnz receives the number of stored entries.  Blocking.
 *   Errors (-1, nothing enqueued, the held W dropped only once every check has passed): topk outside [1, GANMF_ITEMKNN_MAX_TOPK],
 *   col_topk outside [0, GANMF_ITEMKNN_MAX_TOPK], a scale that is negative or not finite, row_scale NULL, a side that has not been
 *   uploaded or is not canonical, a data-parallel handle, a handle of another model. */
int ganmf_p3_fit(ganmf_handle* h, int32_t topk, int32_t col_topk, int normalize, const float* row_scale, const float* col_scale,
                 int64_t* nnz);

/* SLIM-BPR trained on the device (SLIM_BPR/Cython/SLIM_BPR_Cython_Epoch.pyx: the epoch :198-347, the sampler :427-471, get_S
 * :373-421; dense and symmetric storage, not the tree-CSR mode).  All entries need a GANMF_MODEL_ITEMSIM handle; everything is
 * float64, as in the reference.  ganmf_amd/csrc/slim_bpr.hpp states the kernels and the storage in full, counter_draw.hpp the sampler.
 * ganmf_slim_bpr_init: allocates S -- [num_items, num_items], or with symmetric != 0 one cell per unordered pair of items, S[a, b]
 *   and S[b, a] being one value -- and the per-item optimiser state (state0: the AdaGrad / RMSprop cache or Adam's first moment;
 *   state1: Adam's second moment), all zero, and resets the epoch counter and Adam's beta powers (beta_1, beta_2).  The profiles the
 *   samples are drawn from and summed over are indptr / indices (users x items, canonical form: ascending without repeats), or with
 *   indptr = NULL the pattern of side 0 of ganmf_als_set_confidence; the library keeps its own copy.  An earlier training state is
 *   dropped; the held W is not touched.  Errors: -1 for an unknown sgd mode, parameters that are not finite (beta outside [0, 1) for
 *   Adam), profiles that are not canonical, and when no user has a profile that is neither empty nor full (the reference's sampler
 *   would not return); -2 "out of memory", naming the bytes asked for, when an allocation fails: the handle holds no training state
 *   then and stays usable.
 * ganmf_slim_bpr_draw: the samples of the epochs [epoch, epoch + n_epochs), num_users + 1 per epoch (the reference's count with its
 *   batch size of 1), to users / pos / neg [n_epochs * (num_users + 1)].  One launch, one thread per sample; a sample is a pure function
 *   of (seed, epoch, index in the epoch) and the profiles: a uniform user whose profile is neither empty nor full, a uniform item of
 *   the profile, a uniform item outside it.  Training state is not read or changed.
 * ganmf_slim_bpr_run: applies the n samples (users[t], pos[t], neg[t]) with the reference's sequential semantics: for t = 0, 1, ...
 *     x = sum over s in profile(u) of S[i, s] - S[j, s];  g = 1 / (1 + exp(x));  the state of i and j and the step `upd` (the moments
 *     of i only for Adam, whose beta powers advance once per sample);  S[i, s] += lr (upd - lambda_i S[i, s]) for s != i;
 *     S[j, s] -= lr (upd - lambda_j S[j, s]) for s != j.
 *   One workgroup per sample; the sum is a fixed tree: the same bytes on every run.  mode GANMF_SLIM_SEQUENTIAL: one workgroup walks
 *   the list in order.  GANMF_SLIM_LEVELLED (symmetric = 0 only): a sample touches rows i and j of S and the state of i and j only, so
 *   the host sorts the list into levels (ganmf_amd/csrc/level_sched.hpp: level = 1 + the larger level of the last earlier samples that
 *   named i or j) and launches one grid per level; the bytes are those of the sequential route.  GANMF_SLIM_AUTO: levelled when
 *   symmetric = 0.  *n_levels (may be NULL) receives the number of levels, 0 on the sequential route.  n = 0 is allowed.  Errors (-1,
 *   nothing enqueued): ids out of range, pos[t] == neg[t], an unknown mode, LEVELLED with symmetric storage, no training state.
 * ganmf_slim_bpr_epochs: ganmf_slim_bpr_draw of the next n_epochs epochs followed by ganmf_slim_bpr_run of them, the samples staying
 *   on the device (their items are copied back once, for the schedule); advances the epoch counter.
 * ganmf_slim_bpr_finish: get_S and the class's similarityMatrixTopK: the diagonal of S is set to zero; of every row of S the
 *   min(topk, num_items) largest values are selected in float64 (select_topk_nonzero), ties to the smaller id, and the non-zero
 *   ones kept and rounded to float32 (row i of R); of every column of R the min(topk, num_items) largest non-zeros are kept (the
 *   kernels of ganmf_p3_fit's column pass, bit copies).  The handle then holds that matrix as W BY TARGET ITEM, W[i, j] = S[i, j] where kept -- the reference's
 *   orientation: the scores sum S[s, j] over the profile, the training sums S[j, s] -- as after ganmf_itemknn_fit.  S and the state
 *   stay: training continues.  *nnz receives the stored entries.  Errors (-1): topk < 1, min(topk, num_items) above
 *   GANMF_ITEMKNN_MAX_TOPK, no training state.
 * ganmf_slim_bpr_get_state: S as a dense [num_items, num_items] matrix (both halves when symmetric), state0 / state1 [num_items], the
 *   two beta powers the next sample would divide by, the epoch counter.  Every pointer may be NULL. */
enum { GANMF_SLIM_SGD = 0, GANMF_SLIM_ADAGRAD = 1, GANMF_SLIM_RMSPROP = 2, GANMF_SLIM_ADAM = 3 };
enum { GANMF_SLIM_AUTO = 0, GANMF_SLIM_SEQUENTIAL = 1, GANMF_SLIM_LEVELLED = 2 };
int ganmf_slim_bpr_init(ganmf_handle* h, int symmetric, int sgd_mode, double learning_rate, double lambda_i, double lambda_j, double gamma,
                        double beta_1, double beta_2, uint64_t seed, const int64_t* indptr, const int32_t* indices);
int ganmf_slim_bpr_draw(ganmf_handle* h, int64_t epoch, int64_t n_epochs, int32_t* users, int32_t* pos, int32_t* neg);
int ganmf_slim_bpr_run(ganmf_handle* h, const int32_t* users, const int32_t* pos, const int32_t* neg, int64_t n, int mode,
                       int64_t* n_levels);
int ganmf_slim_bpr_epochs(ganmf_handle* h, int64_t n_epochs, int mode, int64_t* n_levels);
int ganmf_slim_bpr_finish(ganmf_handle* h, int32_t topk, int64_t* nnz);
int ganmf_slim_bpr_get_state(ganmf_handle* h, double* S, double* state0, double* state1, double* beta_powers, int64_t* epoch);

/* ---- CFGAN (GANRec/CFGAN.py) on a GANMF_MODEL_CFGAN handle -------------------------------------------------------------------
 * ganmf_cfgan_init: the generator (g_layers >= 1 hidden layers of g_nodes with activation g_act, then a linear layer of width
 *   num_items), the two batch sizes (each clipped to num_users; the larger must not exceed the handle's batch_size), the scheme, the
 *   zero-reconstruction coefficient, the mask sampler's seed and the subset size k_rows[r] of every row (formed by the caller: the
 *   reference sizes BOTH masks by int(n * float(zr_ratio))).  Once per handle.  All parameters start at zero: ganmf_set_tensor.
 * ganmf_cfgan_draw_masks: the device sampler for `epoch`.  For every row and every plane the scheme uses (ZR: the zero-reconstruction
 *   plane; PM: the partial-masking plane; ZP: both, independent) the k_rows[r] non-interactions with the smallest 32-bit keys, ties to
 *   the smaller column; key = high half of the splitmix64 output function over a counter packed from (seed, epoch, plane, row, column).
 *   A pure function of those five: the same bytes on every call and every device.  Needs ganmf_set_urm_csr.
 * ganmf_cfgan_set_masks / ganmf_cfgan_get_masks: the two bit planes [num_users, ceil(num_items / 32)] of 32-bit words, bit (j & 31)
 *   of word (j >> 5) = column j (np.packbits(..., bitorder='little') viewed as little-endian uint32).  set: a NULL plane is cleared;
 *   get: a NULL pointer is skipped.  A set bit on a profile column is the caller's business (the reference's masks never have one).
 * ganmf_cfgan_step: one optimiser step (kind 0: discriminator, 1: generator) on the training rows [row0, row0 + nrows) with the masks
 *   held; *loss (may be NULL) receives the step's loss at the pre-update parameters.
 * ganmf_cfgan_epoch: one epoch in one call, nothing crossing the bus inside it: with draw != 0 the masks of `epoch`, then d_steps
 *   passes of discriminator steps over rows 0.. in slices of d_batch, then g_steps passes of generator steps in slices of g_batch
 *   (last slice ragged, no shuffle); d_losses [d_steps * ceil(U / d_batch)] and g_losses likewise receive every step's loss.  The
 *   same kernels in the same order as the same slices through ganmf_cfgan_step: the same bytes. */
enum { GANMF_CFGAN_ZR = 0, GANMF_CFGAN_PM = 1, GANMF_CFGAN_ZP = 2 };
int ganmf_cfgan_init(ganmf_handle* h, int32_t g_nodes, int32_t g_layers, int g_act, int32_t d_batch, int32_t g_batch, int scheme,
                     float zr_coefficient, uint64_t seed, const int32_t* k_rows);
int ganmf_cfgan_draw_masks(ganmf_handle* h, int64_t epoch);
int ganmf_cfgan_set_masks(ganmf_handle* h, const uint32_t* zr, const uint32_t* pm);
int ganmf_cfgan_get_masks(ganmf_handle* h, uint32_t* zr, uint32_t* pm);
int ganmf_cfgan_step(ganmf_handle* h, int kind, int64_t row0, int32_t nrows, float* loss);
int ganmf_cfgan_epoch(ganmf_handle* h, int64_t epoch, int32_t d_steps, int32_t g_steps, int draw, float* d_losses, float* g_losses);

/* ---- CAAE (GANRec/CAAE.py) on a GANMF_MODEL_CAAE handle ----------------------------------------------------------------------
 * `which` is 0 for G and 1 for G' throughout.  Every draw is a pure function of (seed, epoch, stream, pass / step, index) through the
 * splitmix64 output function (caae_sample.hpp): the same arguments give the same bytes on every call and every device.
 * init: both generators (g_layers >= 1 sigmoid hidden layers of g_units, a sigmoid output layer of width num_items; G' is built like
 *   G, as the reference builds it), the slice length d_bsize of a discriminator step (at most GANMF_CAAE_MAX_D_BSIZE), the users per
 *   generator step m_batch (at most num_users: G draws them distinct), the policy draws per row n_s (the reference's 2 * median profile
 *   length), lmbda, beta, the one learning rate of the three SGD optimisers, the samplers' seed and the size k_rows[u] of every user's
 *   subset Nu (formed by the caller: int(n_free * S)).  Once per handle.  All parameters start at zero: set_tensor.
 * cdf: softmax(r) of generator `which` at its current parameters as an inclusive fp32 prefix sum per row, exactly non-decreasing, and
 *   log sum exp(r).  users == NULL: all users into the handle's resident array (what the negatives are drawn from), rows [0, n)
 *   downloaded; else the n <= m_batch listed users.  cdf_out [n, num_items] and lse_out [n] may be NULL.
 * draw_perm: the order of the nnz stored interactions for `epoch` (position t holds CSR position out[t]); left resident.
 * draw_negatives: draw_perm, then one negative per position for (epoch, pass, which): a 24-bit uniform in [0, 1) searched in the
 *   resident CDF row of the position's user -- the first index whose value is >= it, clamped to num_items - 1.
 * draw_batch: the batch of generator step (epoch, which, step): m_batch users (G: distinct; G': with replacement), for G the bit planes
 *   [m_batch, ceil(num_items / 32)] of Nu in ganmf_cfgan_set_masks' layout -- k_rows[u] non-interactions drawn without replacement with
 *   weights exp(r') of G' at its current parameters, as the k smallest Efraimidis-Spirakis keys -- and n_s policy items per row from
 *   the CDF of generator `which` over the batch's rows, which cdf_out [m_batch, num_items] receives.  Every output may be NULL.
 * get_draws: what the last epoch call drew, by kind and pass / step index (a CDF kind: by user, one row of the resident array).  draw_perm
 *   and draw_negatives write where an epoch keeps its order and its first pass's negatives: read an epoch's draws before calling them.
 * d_step: one discriminator step on `count` <= d_bsize explicit triples; g_step: one step of generator `which` on m_batch explicit
 *   users, Nu planes (G only; NULL: empty) and m_batch * n_s policy items.  *loss (may be NULL): the loss at the pre-step parameters.
 *   Contributions to one row of P, Q or b are summed in ascending position (an item's positives in front of its negatives), without
 *   floating-point atomics: the same arguments leave the same bytes.
 * epoch: one epoch in one call, nothing crossing the bus inside it: the order, both resident CDFs, d_steps passes (the pass's
 *   negatives, then per slice of d_bsize positions a step with G's negatives and a step with G''s), g_steps steps of G and gpr_steps
 *   steps of G', each on its own drawn batch.  d_losses [d_steps * 2 * ceil(nnz / d_bsize)], g_losses [g_steps], gpr_losses [gpr_steps].
 *   The same kernels in the same order as d_step / g_step on the recorded draws: the same bytes. */
#define GANMF_CAAE_MAX_FACTORS 256
#define GANMF_CAAE_MAX_D_BSIZE 16384
enum { GANMF_CAAE_DRAW_PERM = 0, GANMF_CAAE_DRAW_NEG_G = 1, GANMF_CAAE_DRAW_NEG_GPR = 2, GANMF_CAAE_DRAW_USERS_G = 3,
       GANMF_CAAE_DRAW_USERS_GPR = 4, GANMF_CAAE_DRAW_NU = 5, GANMF_CAAE_DRAW_ITEMS_G = 6, GANMF_CAAE_DRAW_ITEMS_GPR = 7,
       GANMF_CAAE_DRAW_CDF_G = 8, GANMF_CAAE_DRAW_CDF_GPR = 9 };
int ganmf_caae_init(ganmf_handle* h, int32_t g_units, int32_t g_layers, int32_t d_bsize, int32_t m_batch, int32_t n_s, float lmbda,
                    float beta, float lr, uint64_t seed, const int32_t* k_rows);
int ganmf_caae_cdf(ganmf_handle* h, int which, const int32_t* users, int32_t n, float* cdf_out, float* lse_out);
int ganmf_caae_draw_perm(ganmf_handle* h, int64_t epoch, int32_t* out);
int ganmf_caae_draw_negatives(ganmf_handle* h, int64_t epoch, int32_t pass, int which, int32_t* out);
int ganmf_caae_draw_batch(ganmf_handle* h, int64_t epoch, int which, int32_t step, int32_t* users, uint32_t* nu, int32_t* items,
                          float* cdf_out);
int ganmf_caae_get_draws(ganmf_handle* h, int kind, int32_t index, void* out, int64_t bytes);
int ganmf_caae_d_step(ganmf_handle* h, const int32_t* users, const int32_t* pos_items, const int32_t* neg_items, int32_t count, float* loss);
int ganmf_caae_g_step(ganmf_handle* h, int which, const int32_t* users, const uint32_t* nu, const int32_t* items, float* loss);
int ganmf_caae_epoch(ganmf_handle* h, int64_t epoch, int32_t d_steps, int32_t g_steps, int32_t gpr_steps, float* d_losses, float* g_losses,
                     float* gpr_losses);

/* Device-resident scoring GEMM timing (no D2H): scores for the first n rows, `iters` launches;
 * returns average milliseconds per launch measured with hipEvents on the handle's stream. */
int ganmf_bench_scores(ganmf_handle* h, int64_t n, int transposed, int32_t iters, float* ms_per_launch);

/* Stand-alone fp32 MFMA GEMM on host buffers, C[M,N] = op(A) . op(B):
 *   a_kmajor = 0: A is [M, K] row-major;  1: A is [K, M] row-major
 *   b_kmajor = 0: B is [N, K] row-major;  1: B is [K, N] row-major
 * tile = 0 auto, 64 or 128; nsplit = 0 auto.  `iters` >= 1 repeats the launch on resident data and
 * returns the average kernel milliseconds in *ms (may be NULL).  Test and bench entry. */
int ganmf_gemm_f32(int device, const float* A, const float* B, float* C, int64_t M, int64_t N,
                   int64_t K, int a_kmajor, int b_kmajor, int tile, int nsplit, int iters, float* ms);

/* The same entry with what only the training step's launches use (tests of their K loops):
 *   a_gather  NULL, or M row ids: row r of the product's A is row a_gather[r] of the [a_rows, K] matrix A (a_kmajor = 0; needs a
 *             16-wave 64 x 64 plan: tile = 64 with GANMF_TUNE kg=4,ring=3)
 *   bk        0 auto, 32: the 32-deep K-tile of the 4-wave staged split-bf16 kernel (GANMF_MFMA=bf16x3, tile = 64)
 *   adam_m    NULL, or [M, N]: the product runs unsplit behind the fused TF-Adam epilogue on theta = m = v = 0 with lr_t = 1e-3 and
 *             no L2 term; C returns the updated theta and adam_m the first moment, (1 - beta1) x the product */
int ganmf_gemm_f32_ex(int device, const float* A, const float* B, float* C, int64_t M, int64_t N,
                      int64_t K, int a_kmajor, int b_kmajor, int tile, int nsplit, int iters, float* ms,
                      const int32_t* a_gather, int64_t a_rows, int bk, float* adam_m);

/* Host-only helper of the checkpoint writer/reader (ganmf_amd/tf_bundle.py): CRC-32C (Castagnoli), the
 * checksum tf.train.Saver stores per tensor and per table block (GANMF.py:309-314,337-339).  Pass crc = 0
 * to start; feed the previous return value to continue over a second buffer. */
uint32_t ganmf_crc32c(uint32_t crc, const void* data, uint64_t n);

int ganmf_device_count(void);
/* Bytes of device memory the library holds in this process, over all handles and all devices: what every allocation asked for (at
 * least 16 bytes each), added when it is made and subtracted when it is freed.  Pinned host staging is not counted.  After the last
 * ganmf_destroy it is back at its value before the first ganmf_create (tests/test_gpu_device_memory.py). */
int64_t ganmf_live_device_bytes(void);
int ganmf_abi_version(void);
const char* ganmf_last_error(void);

/* ---- MF-BPR and FunkSVD trained on the device (MatrixFactorization/Cython/MatrixFactorization_Cython_Epoch.pyx: the epochs :287-389
 * and :614-696, adaptive_gradient :760-798, the samplers :803-910) on a GANMF_MODEL_MF handle.  float64, as in the reference;
 * ganmf_amd/csrc/mf_sgd.hpp states the kernels and the summation orders in full, counter_draw.hpp the sampler.  New entries; no structure or signature
 * changed: GANMF_ABI_VERSION stays.
 * init: allocates W [num_users, k], H [num_items, k], the three biases and two optimiser values per element, in float64, with
 *   k = the handle's num_factors - 2 use_bias (a biased model publishes two more columns, see publish); W and H start as
 *   user_factors / item_factors, everything else as zero.  (indptr, indices, ratings) is the users x items CSR the samples are drawn
 *   from: indices ascending without repeats inside a row (-1 otherwise), every rating finite.  The rates are used as the doubles
 *   given (the caller rounds them to float32, as the reference's C float members do); gamma = 0.995, beta_1 = 0.9, beta_2 = 0.999.
 *   item_reg is stored and never read (the reference's item gradient uses positive_reg).  GANMF_MF_SGD_BPR refuses use_bias.  Errors
 *   (-1, nothing allocated, a state held before is kept): unknown algorithm or mode, a value that is not finite, a quota outside
 *   [0, 1), more than GANMF_MF_SGD_MAX_FACTORS columns, no user whose profile is neither empty nor full.  -2 "out of memory: ...
 *   needs N bytes" when an allocation fails; the handle stays usable.
 * draw: the samples of the epochs [epoch, epoch + n_epochs): (num_users / batch_size + 1) batch_size per epoch for BPR,
 *   (nnz / batch_size + 1) batch_size for FunkSVD.  A pure function of (seed, epoch, index) and the profiles.  BPR fills neg_items,
 *   FunkSVD ratings (the other may be NULL).  Nothing of the state moves.
 * run: applies the n samples in mini-batches of batch_size (the last one may be shorter) with the reference's semantics: per batch
 *   one scalar, the mean over the batch of 1 / (1 + exp(x_uij)) or of rating - prediction at frozen parameters, then the samples in
 *   list order, each reading the current rows.  GANMF_MF_SGD_SEQUENTIAL: one wave walks a batch in order (2 launches per batch).
 *   GANMF_MF_SGD_LEVELLED (and AUTO): the host sorts every batch into levels (ganmf_amd/csrc/level_sched.hpp) and launches one grid
 *   per level; the bytes are those of the sequential route.  *n_levels (may be NULL): the largest level count of a batch (0 on the
 *   sequential route).  Errors (-1, nothing enqueued): an id out of range, a BPR sample with equal items, a rating that is not
 *   finite, batch_size outside [1, GANMF_MF_SGD_MAX_BATCH].
 * epochs: draw of the next n_epochs epochs followed by run of them, the samples staying on the device (the levelled route copies
 *   their ids back once per epoch); advances the epoch counter.  *n_levels as for run, over all batches.
 * publish: rounds the float64 state into the handle's float32 factor tensors, with use_bias as U' = [W | USER_bias + GLOBAL_bias | 1]
 *   and V' = [H | 1 | ITEM_bias]: every scoring, ranking, evaluation and best-slot entry then serves W H^T + the three biases.
 * get_state / set_state: the three blocks (parameters, state0, state1), each num_users k + num_items k + num_users + num_items + 1
 *   values laid out [W | H | USER_bias | ITEM_bias | GLOBAL_bias], Adam's two beta powers and the epoch counter.  A NULL pointer is
 *   skipped; set_state keeps the counter for epoch = -1. */
#define GANMF_MF_SGD_MAX_FACTORS 1024
#define GANMF_MF_SGD_MAX_BATCH (1 << 20)
enum { GANMF_MF_SGD_BPR = 0, GANMF_MF_SGD_FUNK = 1 };
enum { GANMF_MF_SGD_AUTO = 0, GANMF_MF_SGD_SEQUENTIAL = 1, GANMF_MF_SGD_LEVELLED = 2 };
int ganmf_mf_sgd_init(ganmf_handle* h, int algorithm, int use_bias, int sgd_mode, double learning_rate, double user_reg, double item_reg,
                      double positive_reg, double negative_reg, double bias_reg, double negative_interactions_quota, uint64_t seed,
                      const int64_t* indptr, const int32_t* indices, const double* ratings, const double* user_factors,
                      const double* item_factors);
int ganmf_mf_sgd_draw(ganmf_handle* h, int64_t epoch, int64_t n_epochs, int64_t batch_size, int32_t* users, int32_t* items,
                      int32_t* neg_items, double* ratings);
int ganmf_mf_sgd_run(ganmf_handle* h, const int32_t* users, const int32_t* items, const int32_t* neg_items, const double* ratings, int64_t n,
                     int64_t batch_size, int route, int64_t* n_levels);
int ganmf_mf_sgd_epochs(ganmf_handle* h, int64_t n_epochs, int64_t batch_size, int route, int64_t* n_levels);
int ganmf_mf_sgd_publish(ganmf_handle* h);
int ganmf_mf_sgd_get_state(ganmf_handle* h, double* params, double* state0, double* state1, double* beta_powers, int64_t* epoch);
int ganmf_mf_sgd_set_state(ganmf_handle* h, const double* params, const double* state0, const double* state1, const double* beta_powers,
                           int64_t epoch);

#ifdef __cplusplus
}
#endif
#endif /* GANMF_HIP_H */
