"""Thin object wrapper of one libganmf_hip handle (one GPU).  No arithmetic happens here."""
import ctypes as C

import numpy as np

from . import _lib as L


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Engine:
    def __init__(self, num_users, num_items, num_factors, emb_dim, batch_size, d_lr=1e-4, g_lr=1e-4, d_reg=0.0,
                 g_reg=0.0, m=1.0, recon_coefficient=1e-2, model=L.MODEL_GANMF, d_layers=1, d_act="linear",
                 device=0, world_size=1, rank=0, row_offset=0, mfma=None):
        """mfma: None/"auto" (fp32-accurate, kernel chosen per GEMM), "f32" (plain fp32 MFMA everywhere) or "bf16"
        (operands rounded to bf16, fp32 accumulate and fp32 master weights/Adam: the mixed-precision variant)."""
        self.lib = L.load_library()
        if self.lib.ganmf_device_count() < 1:
            raise L.GanmfError("no HIP device visible: libganmf_hip has no CPU fallback")
        cfg = L.Cfg(abi_version=L.ABI_VERSION, model=model, num_users=num_users, num_items=num_items,
                    num_factors=num_factors, emb_dim=emb_dim, d_layers=d_layers, d_act=L.ACT[d_act],
                    batch_size=batch_size, d_lr=d_lr, g_lr=g_lr, d_reg=d_reg, g_reg=g_reg, m=m,
                    recon_coefficient=recon_coefficient, device=device, world_size=world_size, rank=rank,
                    row_offset=row_offset, flags=L.MFMA_FLAGS[mfma])
        self.cfg = cfg
        self.h = C.c_void_p()
        L.check(self.lib.ganmf_create(C.byref(cfg), C.byref(self.h)), "ganmf_create")
        self.num_users, self.num_items = num_users, num_items
        self.batch_size = min(batch_size, num_users)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.ganmf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data -------------------------------------------------------------------------------
    def set_urm(self, urm_csr):
        urm = urm_csr.tocsr()
        urm.sum_duplicates()
        urm.sort_indices()
        indptr = np.ascontiguousarray(urm.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(urm.indices, dtype=np.int32)
        data = np.ascontiguousarray(urm.data, dtype=np.float32)
        self._nnz = int(indptr[-1])      # (the CAAE entries size their host buffers by the stored interactions)
        L.check(self.lib.ganmf_set_urm_csr(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices),
                                           _f32p(data), urm.shape[0], urm.shape[1]), "ganmf_set_urm_csr")

    def shape(self, tid):
        r, c = C.c_int64(), C.c_int64()
        L.check(self.lib.ganmf_tensor_shape(self.h, tid, C.byref(r), C.byref(c)), "ganmf_tensor_shape")
        return r.value, c.value

    def set_tensor(self, tid, arr, slot=L.SLOT_PARAM):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        L.check(self.lib.ganmf_set_tensor(self.h, tid, slot, _f32p(a), a.size), "ganmf_set_tensor")

    def get_tensor(self, tid, slot=L.SLOT_PARAM):
        r, c = self.shape(tid)
        out = np.empty((r, c), dtype=np.float32)
        L.check(self.lib.ganmf_get_tensor(self.h, tid, slot, _f32p(out), out.size), "ganmf_get_tensor")
        return out

    def adam_powers(self):
        out = np.empty(4, dtype=np.float32)
        L.check(self.lib.ganmf_get_adam_powers(self.h, _f32p(out)), "ganmf_get_adam_powers")
        return out

    def set_adam_powers(self, p):
        a = np.ascontiguousarray(p, dtype=np.float32)
        L.check(self.lib.ganmf_set_adam_powers(self.h, _f32p(a)), "ganmf_set_adam_powers")

    # -- training ---------------------------------------------------------------------------
    def train_epoch(self, perm, d_steps=1, g_steps=1, steps_per_pass=0, global_batch_rows=None):
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        n = perm.size
        per_pass = max(-(-n // self.batch_size), steps_per_pass)
        dl = np.zeros(max(d_steps * per_pass, 1), dtype=np.float32)
        gl = np.zeros(max(g_steps * per_pass, 1), dtype=np.float32)
        gb = None
        if global_batch_rows is not None:
            gb = np.ascontiguousarray(global_batch_rows, dtype=np.int32)
            assert gb.size == per_pass
        L.check(self.lib.ganmf_train_epoch(self.h, _i32p(perm), n, d_steps, g_steps, steps_per_pass,
                                           _i32p(gb) if gb is not None else None, _f32p(dl), _f32p(gl)),
                "ganmf_train_epoch")
        return dl[:d_steps * per_pass], gl[:g_steps * per_pass]

    def train_epoch_ragged(self, perm, local_batch_rows, global_batch_rows, d_steps=1, g_steps=1):
        """Slices of given sizes (ganmf_train_epoch_ragged): slice i = the next local_batch_rows[i] rows of `perm`, part of a
        global minibatch of global_batch_rows[i] rows (row-sharded fit(), ganmf_amd/dist.py)."""
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        lb = np.ascontiguousarray(local_batch_rows, dtype=np.int32)
        gb = np.ascontiguousarray(global_batch_rows, dtype=np.int32)
        assert lb.size == gb.size and int(lb.sum()) == perm.size
        per_pass = lb.size
        dl = np.zeros(max(d_steps * per_pass, 1), dtype=np.float32)
        gl = np.zeros(max(g_steps * per_pass, 1), dtype=np.float32)
        L.check(self.lib.ganmf_train_epoch_ragged(self.h, _i32p(perm), perm.size, d_steps, g_steps, per_pass, _i32p(gb),
                                                  _i32p(lb), _f32p(dl), _f32p(gl)), "ganmf_train_epoch_ragged")
        return dl[:d_steps * per_pass], gl[:g_steps * per_pass]

    def train_step(self, kind, uids):
        u = np.ascontiguousarray(uids, dtype=np.int32)
        loss = C.c_float()
        L.check(self.lib.ganmf_train_step(self.h, kind, _i32p(u), u.size, C.byref(loss)), "ganmf_train_step")
        return np.float32(loss.value)

    def scores(self, ids, transposed=False):
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        width = self.num_users if transposed else self.num_items
        out = np.empty((ids.size, width), dtype=np.float32)
        if ids.size:
            L.check(self.lib.ganmf_scores(self.h, _i32p(ids), ids.size, int(transposed), _f32p(out)), "ganmf_scores")
        return out

    def set_seen(self, urm_eval_csr):
        """URM_train in evaluation orientation (rows = users the evaluator asks about)."""
        urm = urm_eval_csr.tocsr()
        urm.sort_indices()
        indptr = np.ascontiguousarray(urm.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(urm.indices, dtype=np.int32)
        L.check(self.lib.ganmf_set_seen_csr(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices),
                                            urm.shape[0], urm.shape[1]), "ganmf_set_seen_csr")

    def set_score_filter(self, items_to_compute=None, mask_cold=False):
        """MF contract (BaseMatrixFactorizationRecommender.py:113-119,128-143) for every later scores / recommend / evaluate
        call: only `items_to_compute` keep their scores (the others -inf); rows that are empty in the set_seen() matrix score
        -inf everywhere."""
        if items_to_compute is None or len(items_to_compute) == 0:
            L.check(self.lib.ganmf_set_score_filter(self.h, None, 0, int(bool(mask_cold))), "ganmf_set_score_filter")
            return
        items = np.ascontiguousarray(np.asarray(items_to_compute).reshape(-1), dtype=np.int32)
        L.check(self.lib.ganmf_set_score_filter(self.h, _i32p(items), len(items), int(bool(mask_cold))), "ganmf_set_score_filter")

    def set_items_to_ignore(self, items=None):
        """Columns that score -inf in everything that ranks -- recommend*, evaluate* -- until the list is cleared (None or empty),
        on top of set_score_filter (ganmf_set_items_to_ignore; BaseRecommender.py:84-86, 207-211).  scores() is not affected."""
        if items is None or len(items) == 0:
            L.check(self.lib.ganmf_set_items_to_ignore(self.h, None, 0), "ganmf_set_items_to_ignore")
            return
        items = np.ascontiguousarray(np.asarray(items).reshape(-1), dtype=np.int32)
        L.check(self.lib.ganmf_set_items_to_ignore(self.h, _i32p(items), len(items)), "ganmf_set_items_to_ignore")

    def recommend(self, ids, cutoff, transposed=False, remove_seen=True):
        """device top-k: returns (items [n, cutoff] int32 with -1 padding, scores [n, cutoff])"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        items = np.empty((ids.size, cutoff), dtype=np.int32)
        vals = np.empty((ids.size, cutoff), dtype=np.float32)
        if ids.size:
            L.check(self.lib.ganmf_recommend(self.h, _i32p(ids), ids.size, int(transposed), int(cutoff), int(remove_seen),
                                             _i32p(items), _f32p(vals)), "ganmf_recommend")
        return items, vals

    def set_test(self, urm_test_csr, gains):
        """URM_test in evaluation orientation, column indices sorted inside each row; `gains` = 2^rating - 1 per stored
        entry (float64, same order as urm_test_csr.data)."""
        urm = urm_test_csr.tocsr()
        assert urm.has_sorted_indices
        indptr = np.ascontiguousarray(urm.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(urm.indices, dtype=np.int32)
        g = np.ascontiguousarray(gains, dtype=np.float64)
        assert g.size == indices.size
        L.check(self.lib.ganmf_set_test_csr(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices),
                                            _f64p(g), urm.shape[0], urm.shape[1]), "ganmf_set_test_csr")

    @staticmethod
    def _eval_args(ids, cutoffs, disc, ideal_cum):
        """the arguments every evaluate* shares as contiguous arrays (ids, cut-offs int32; disc, ideal_cum float64), the last two
        checked to reach the largest cut-off"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        cut = np.ascontiguousarray(cutoffs, dtype=np.int32).ravel()
        K = int(cut.max())
        disc = np.ascontiguousarray(disc, dtype=np.float64).ravel()
        ideal = np.ascontiguousarray(ideal_cum, dtype=np.float64)
        assert disc.size >= K and ideal.shape == (ids.size, K)
        return ids, cut, disc, ideal

    def _counts_arg(self, counts, n_cutoffs, transposed):
        """(`counts`, or a new zero array when None: [n_cutoffs, width] int64; its pointer)"""
        width = self.num_users if transposed else self.num_items
        if counts is None:
            counts = np.zeros((n_cutoffs, width), dtype=np.int64)
        assert counts.dtype == np.int64 and counts.shape == (n_cutoffs, width) and counts.flags.c_contiguous
        return counts, counts.ctypes.data_as(C.POINTER(C.c_int64))

    def evaluate(self, ids, cutoffs, disc, ideal_cum, transposed=False, remove_seen=True):
        """Sums over the users `ids` of the nine ranking metrics (L.EVAL_METRICS) per cut-off, formed on the device from
        the device's own top-k lists: returns a [len(cutoffs), 9] float64 array."""
        ids, cut, disc, ideal = self._eval_args(ids, cutoffs, disc, ideal_cum)
        out = np.zeros((cut.size, len(L.EVAL_METRICS)), dtype=np.float64)
        if ids.size:
            L.check(self.lib.ganmf_evaluate(self.h, _i32p(ids), ids.size, int(transposed), int(remove_seen), _i32p(cut), cut.size,
                                            _f64p(disc), _f64p(ideal), _f64p(out)), "ganmf_evaluate")
        return out

    def set_test_ratings(self, ratings):
        """float32 rating of every stored entry of the set_test() matrix, in its order (RMSE of evaluate_full)"""
        r = np.ascontiguousarray(ratings, dtype=np.float32).ravel()
        L.check(self.lib.ganmf_set_test_ratings(self.h, _f32p(r), r.size), "ganmf_set_test_ratings")

    def set_eval_item_weights(self, novelty, popularity):
        """per-item novelty term and normalised popularity of the evaluation width (ganmf_amd.evaluation.popularity_weights)"""
        nov = np.ascontiguousarray(novelty, dtype=np.float64).ravel()
        pop = np.ascontiguousarray(popularity, dtype=np.float64).ravel()
        assert nov.size == pop.size
        L.check(self.lib.ganmf_set_eval_item_weights(self.h, _f64p(nov), _f64p(pop), nov.size), "ganmf_set_eval_item_weights")

    def evaluate_full(self, ids, cutoffs, disc, ideal_cum, transposed=False, remove_seen=True, counts=None):
        """evaluate() plus RMSE, NOVELTY, AVERAGE_POPULARITY and non-empty-list sums (L.EVAL_FULL_METRICS, [len(cutoffs), 13]
        float64) and the per-item counts of the lists cut at each cut-off, ADDED into `counts` ([len(cutoffs), width] int64,
        a new zero array when None).  Returns (sums, counts)."""
        ids, cut, disc, ideal = self._eval_args(ids, cutoffs, disc, ideal_cum)
        counts, cp = self._counts_arg(counts, cut.size, transposed)
        out = np.zeros((cut.size, len(L.EVAL_FULL_METRICS)), dtype=np.float64)
        if ids.size:
            L.check(self.lib.ganmf_evaluate_full(self.h, _i32p(ids), ids.size, int(transposed), int(remove_seen), _i32p(cut),
                                                 cut.size, _f64p(disc), _f64p(ideal), _f64p(out), cp), "ganmf_evaluate_full")
        return out, counts

    def set_candidates(self, candidates_csr):
        """Per-row candidate lists in evaluation orientation (ganmf_set_candidates_csr): the stored entries of a scipy matrix,
        in any order and with repeats (the library sorts and de-duplicates the rows); None drops the held matrix."""
        if candidates_csr is None:
            L.check(self.lib.ganmf_set_candidates_csr(self.h, None, None, 0, 0), "ganmf_set_candidates_csr")
            return
        m = candidates_csr.tocsr()
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        L.check(self.lib.ganmf_set_candidates_csr(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices),
                                                  m.shape[0], m.shape[1]), "ganmf_set_candidates_csr")

    def recommend_candidates(self, ids, cutoff, transposed=False, remove_seen=True):
        """device top-k of every row among its own candidates: (items [n, cutoff] int32 with -1 padding, scores [n, cutoff])"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        items = np.empty((ids.size, cutoff), dtype=np.int32)
        vals = np.empty((ids.size, cutoff), dtype=np.float32)
        if ids.size:
            L.check(self.lib.ganmf_recommend_candidates(self.h, _i32p(ids), ids.size, int(transposed), int(cutoff), int(remove_seen),
                                                        _i32p(items), _f32p(vals)), "ganmf_recommend_candidates")
        return items, vals

    def evaluate_candidates(self, ids, cutoffs, disc, ideal_cum, transposed=False, remove_seen=True, counts=None, full=False):
        """evaluate() / evaluate_full() with every row ranked among its own candidates (ganmf_evaluate_candidates).  full=False:
        the [len(cutoffs), 9] sums.  full=True: (the [len(cutoffs), 13] sums, `counts` with the lists' per-item counts added)."""
        ids, cut, disc, ideal = self._eval_args(ids, cutoffs, disc, ideal_cum)
        cp = None
        if full:
            counts, cp = self._counts_arg(counts, cut.size, transposed)
        out = np.zeros((cut.size, len(L.EVAL_FULL_METRICS if full else L.EVAL_METRICS)), dtype=np.float64)
        if ids.size:
            L.check(self.lib.ganmf_evaluate_candidates(self.h, _i32p(ids), ids.size, int(transposed), int(remove_seen), _i32p(cut),
                                                       cut.size, _f64p(disc), _f64p(ideal), _f64p(out), cp),
                    "ganmf_evaluate_candidates")
        return (out, counts) if full else out

    def evaluate_groups(self, ids, cutoffs, disc, ideal_cum, group_of, n_groups, transposed=False, remove_seen=True,
                        candidates=False, per_user=False):
        """evaluate() (candidates=False) or evaluate_candidates() (candidates=True) per group of users (ganmf_evaluate_groups):
        group_of[i] in [-1, n_groups) is the group of ids[i], -1 = in no group (None with n_groups = 0: per-user values only).
        Returns (sums [n_groups, len(cutoffs), 9] float64 over each group's members, sizes [n_groups] int64, the
        [len(ids), len(cutoffs), 9] per-user values in the order of `ids` when per_user=True, else None)."""
        ids, cut, disc, ideal = self._eval_args(ids, cutoffs, disc, ideal_cum)
        G = int(n_groups)
        grp = None
        if group_of is not None:
            grp = np.ascontiguousarray(group_of, dtype=np.int32).ravel()
            assert grp.size == ids.size
        sums = np.zeros((max(G, 0), cut.size, len(L.EVAL_METRICS)), dtype=np.float64)
        sizes = np.zeros(max(G, 0), dtype=np.int64)
        users = np.zeros((ids.size, cut.size, len(L.EVAL_METRICS)), dtype=np.float64) if per_user else None
        if ids.size:
            L.check(self.lib.ganmf_evaluate_groups(self.h, _i32p(ids), ids.size, int(transposed), int(remove_seen), int(candidates),
                                                   _i32p(cut), cut.size, _f64p(disc), _f64p(ideal),
                                                   _i32p(grp) if grp is not None else None, G,
                                                   _f64p(sums) if G > 0 else None,
                                                   sizes.ctypes.data_as(C.POINTER(C.c_int64)) if G > 0 else None,
                                                   _f64p(users) if users is not None else None), "ganmf_evaluate_groups")
        return sums, sizes, users

    def set_item_diversity(self, matrix=None):
        """The [width, width] float32 item diversity matrix of evaluate_diversity, resident until replaced; None drops it
        (ganmf_set_item_diversity).  MemoryError when it would take over a quarter of the free device memory."""
        if matrix is None:
            L.check(self.lib.ganmf_set_item_diversity(self.h, None, 0), "ganmf_set_item_diversity")
            return
        m = np.ascontiguousarray(matrix, dtype=np.float32)
        assert m.ndim == 2 and m.shape[0] == m.shape[1]
        L.check(self.lib.ganmf_set_item_diversity(self.h, _f32p(m), m.shape[0]), "ganmf_set_item_diversity")

    def evaluate_diversity(self, ids, cutoffs, transposed=False, remove_seen=True, candidates=False, per_user=False):
        """Sums over the users `ids` of the intra-list diversity of their ranked lists per cut-off (ganmf_evaluate_diversity; the
        ranking of evaluate(), or with candidates=True of evaluate_candidates()): a [len(cutoffs)] float64 array, with
        per_user=True (that, the [len(ids), len(cutoffs)] per-user values).  A list shorter than two items at a cut-off has value 0."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        cut = np.ascontiguousarray(cutoffs, dtype=np.int32).ravel()
        sums = np.zeros(cut.size, dtype=np.float64)
        users = np.zeros((ids.size, cut.size), dtype=np.float64) if per_user else None
        if ids.size:
            L.check(self.lib.ganmf_evaluate_diversity(self.h, _i32p(ids), ids.size, int(transposed), int(remove_seen), int(candidates),
                                                      _i32p(cut), cut.size, _f64p(sums),
                                                      _f64p(users) if users is not None else None), "ganmf_evaluate_diversity")
        return (sums, users) if per_user else sums

    def score_similarity(self, ids, transposed=False, pool=None, return_matrix=False):
        """Cosine similarity of the (unfiltered) score rows `ids` among themselves, formed on the device (ganmf_score_similarity;
        the computation under AblationStudy.py:88-92,113-117).  Returns a dict: mean and std (population, as np.mean / np.std of
        the [n, n] matrix), n, zero_rows (rows of norm 0: similarity 0 with every row, themselves included), sum_d / sum_d2 (the
        float64 sums of c - 1 and (c - 1)^2 the two are formed from); with pool=P also `pooled`, the [P, P] block means (row i in
        bin i * P // n, 1 <= P <= min(n, 1024)); with return_matrix=True also `matrix`, the [n, n] float32 similarities."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        n = ids.size
        sums = np.zeros(4, dtype=np.float64)
        pooled = matrix = None
        if pool is not None:      # (an invalid pool is refused by the library: give it a buffer it will not write)
            p = int(pool)
            pooled = np.empty((p, p) if 1 <= p <= min(n, 1024) else (1, 1), dtype=np.float32)
        if return_matrix:
            matrix = np.empty((n, n), dtype=np.float32)
        L.check(self.lib.ganmf_score_similarity(self.h, _i32p(ids), n, int(transposed), int(pool) if pool is not None else 0,
                                                _f64p(sums),
                                                _f32p(pooled) if pooled is not None else None,
                                                _f32p(matrix) if matrix is not None else None), "ganmf_score_similarity")
        md = sums[0] / (float(n) * n)
        out = dict(mean=1.0 + md, std=float(np.sqrt(max(sums[1] / (float(n) * n) - md * md, 0.0))), n=n, zero_rows=int(sums[2]),
                   sum_d=float(sums[0]), sum_d2=float(sums[1]))
        if pooled is not None:
            out["pooled"] = pooled
        if matrix is not None:
            out["matrix"] = matrix
        return out

    def discriminate(self, rows, generated=False, features=True, value=True, block=None):
        """The discriminator's view of the generator rows `rows` (training orientation), formed on the device (ganmf_discriminate):
        of their stored profiles, or with generated=True of the unfiltered generated ones U[rows] . V^T.  Returns (features, value),
        None for the one not asked for.  GANMF: the codes E [n, emb_dim] float32 and the per-row energies mean_j (dec(E) - x)_j^2 [n]
        float64; DisGANMF: the last hidden layer's output [n, d_nodes] and the logits [n].  block: rows per block of the call's loop
        (None: what a quarter of the free device memory holds)."""
        ids = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        if not (features or value):
            raise ValueError("discriminate: neither features nor value asked for")
        feat = np.empty((ids.size, int(self.cfg.emb_dim)), dtype=np.float32) if features else None
        val = np.empty(ids.size, dtype=np.float64) if value else None
        L.check(self.lib.ganmf_set_discriminate_block(self.h, 0 if block is None else int(block)), "ganmf_set_discriminate_block")
        try:
            L.check(self.lib.ganmf_discriminate(self.h, _i32p(ids), ids.size, int(bool(generated)),
                                                _f32p(feat) if feat is not None else None,
                                                _f64p(val) if val is not None else None), "ganmf_discriminate")
        finally:
            if block is not None:
                self.lib.ganmf_set_discriminate_block(self.h, 0)
        return feat, val

    # -- implicit ALS (ganmf_als_*) -------------------------------------------------------------
    def set_confidence(self, side, csr):
        """One side of the handle's weighted sparse matrix (ganmf_als_set_confidence): side 0 a users x items CSR, side 1 its
        transpose, items x users; the stored values are the confidences c themselves for ALS, the URM's data for pure_svd (float32)."""
        m = csr.tocsr()
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        conf = np.ascontiguousarray(m.data, dtype=np.float32)
        L.check(self.lib.ganmf_als_set_confidence(self.h, int(side), indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices),
                                                  _f32p(conf), m.shape[0], m.shape[1]), "ganmf_als_set_confidence")

    def als_half_sweep(self, side, reg):
        """One ALS half sweep on the device (ganmf_als_half_sweep): side 0 rewrites the user factors of every user with a stored
        entry from the item factors, side 1 the item factors from the user factors."""
        L.check(self.lib.ganmf_als_half_sweep(self.h, int(side), float(reg)), "ganmf_als_half_sweep")

    def pure_svd(self, omega, n_iter):
        """Randomized truncated SVD of the matrix uploaded by set_confidence (side 0 the URM, side 1 its transpose) into the two
        factor tensors (ganmf_pure_svd): omega is the [min(num_users, num_items), n_random] test matrix, n_iter the number of
        power iterations.  Returns the num_factors singular values (float32)."""
        om = np.ascontiguousarray(omega, dtype=np.float32)
        assert om.ndim == 2
        sigma = np.empty(int(self.cfg.num_factors), dtype=np.float32)
        L.check(self.lib.ganmf_pure_svd(self.h, _f32p(om), int(om.shape[1]), int(n_iter), _f32p(sigma)), "ganmf_pure_svd")
        return sigma

    # -- NMF (ganmf_nmf_*): W = T_USER_EMB, H^T = T_ITEM_EMB as set_tensor left them, X from set_confidence ----------
    def nmf_mu(self, beta_loss, n_iter, update_H=True, error=True):
        """n_iter iterations of sklearn's multiplicative update on the device (ganmf_nmf_mu); beta_loss is L.NMF_FROBENIUS or
        L.NMF_KULLBACK_LEIBLER, update_H=False runs the W half only.  Returns the error after the last iteration (float), or None."""
        err = C.c_double(0.0)
        L.check(self.lib.ganmf_nmf_mu(self.h, int(beta_loss), int(n_iter), int(bool(update_H)), C.byref(err) if error else None),
                "ganmf_nmf_mu")
        return float(err.value) if error else None

    def nmf_cd(self, perms, update_H=True):
        """One coordinate-descent iteration per row of perms [n_iter, 2 if update_H else 1, num_factors] on the device (ganmf_nmf_cd):
        a permutation per half, W half first.  Returns every iteration's violation (float64 [n_iter])."""
        k, halves = int(self.cfg.num_factors), 2 if update_H else 1
        pm = np.ascontiguousarray(perms, dtype=np.int32).reshape(-1, halves, k)
        viol = np.zeros(max(pm.shape[0], 1), dtype=np.float64)
        L.check(self.lib.ganmf_nmf_cd(self.h, _i32p(pm), int(pm.shape[0]), int(bool(update_H)), _f64p(viol)), "ganmf_nmf_cd")
        return viol[:pm.shape[0]]

    def nmf_error(self, beta_loss):
        """sklearn's _beta_divergence(X, W, H, beta_loss, square_root=True) of the factors as they stand (ganmf_nmf_error)"""
        err = C.c_double(0.0)
        L.check(self.lib.ganmf_nmf_error(self.h, int(beta_loss), C.byref(err)), "ganmf_nmf_error")
        return float(err.value)

    # -- item-based nearest neighbours (ganmf_itemknn_*, a MODEL_ITEMSIM engine) ------------------
    def itemknn_fit(self, kind, topk, shrink=0.0, p0=1.0, p1=1.0, den_a=None, den_b=None):
        """The item similarity matrix from the matrix uploaded by set_confidence (side 0 the weighted URM, side 1 its transpose),
        left on the device (ganmf_itemknn_fit): kind is one of L.ITEMKNN_*, den_a / den_b the per-item float32 terms of its
        denominator (None where the kind reads none).  Returns the number of stored similarities."""
        a = None if den_a is None else np.ascontiguousarray(den_a, dtype=np.float32).ravel()
        b = None if den_b is None else np.ascontiguousarray(den_b, dtype=np.float32).ravel()
        assert all(v is None or v.size == self.num_items for v in (a, b))
        nnz = C.c_int64(0)
        L.check(self.lib.ganmf_itemknn_fit(self.h, int(kind), int(topk), float(shrink), float(p0), float(p1),
                                           _f32p(a) if a is not None else None, _f32p(b) if b is not None else None,
                                           C.byref(nnz)), "ganmf_itemknn_fit")
        self._knn_nnz = int(nnz.value)
        return self._knn_nnz

    def userknn_fit(self, kind, topk, shrink=0.0, p0=1.0, p1=1.0, den_a=None, den_b=None):
        """The user similarity matrix from side 0 of set_confidence (the weighted URM, users x items), left on the device by row
        (ganmf_userknn_fit): itemknn_fit with the sides exchanged, den_a / den_b the per-USER float32 terms.  Returns the number
        of stored similarities."""
        a = None if den_a is None else np.ascontiguousarray(den_a, dtype=np.float32).ravel()
        b = None if den_b is None else np.ascontiguousarray(den_b, dtype=np.float32).ravel()
        assert all(v is None or v.size == self.num_users for v in (a, b))
        nnz = C.c_int64(0)
        L.check(self.lib.ganmf_userknn_fit(self.h, int(kind), int(topk), float(shrink), float(p0), float(p1),
                                           _f32p(a) if a is not None else None, _f32p(b) if b is not None else None,
                                           C.byref(nnz)), "ganmf_userknn_fit")
        self._knn_nnz = int(nnz.value)
        return self._knn_nnz

    def p3_fit(self, topk, row_scale, col_scale=None, normalize=False, col_topk=None):
        """The P3alpha / RP3beta matrix from the uploads of set_confidence -- side 0 the URM the scores are formed from, side 1 the
        transition weights Pui^alpha by item -- left on the device (ganmf_p3_fit): row_scale [num_items] = (1 / deg_i)^alpha,
        col_scale [num_items] = deg_j^-beta or None, normalize: the rows divided by their L1 norm between the two selections,
        col_topk: the second, column-wise selection (None: topk; 0: none).  Returns the number of stored weights."""
        a = np.ascontiguousarray(row_scale, dtype=np.float32).ravel()
        b = None if col_scale is None else np.ascontiguousarray(col_scale, dtype=np.float32).ravel()
        assert all(v is None or v.size == self.num_items for v in (a, b))
        nnz = C.c_int64(0)
        L.check(self.lib.ganmf_p3_fit(self.h, int(topk), int(topk if col_topk is None else col_topk), int(bool(normalize)),
                                      _f32p(a), _f32p(b) if b is not None else None, C.byref(nnz)), "ganmf_p3_fit")
        self._knn_nnz = int(nnz.value)
        return self._knn_nnz

    # -- SLIM-BPR (ganmf_slim_bpr_*, a MODEL_ITEMSIM engine) ----------------------------------------
    def slim_bpr_init(self, symmetric=True, sgd_mode="adagrad", learning_rate=1e-4, lambda_i=0.0, lambda_j=0.0, gamma=0.995,
                      beta_1=0.9, beta_2=0.999, seed=0, profiles=None):
        """Zeroed float64 S (one cell per unordered pair when symmetric) and optimiser state on the device (ganmf_slim_bpr_init).
        profiles: the users x items CSR the samples are drawn from and summed over (canonical form); None: the pattern of side 0."""
        if sgd_mode not in L.SLIM_SGD_MODES:
            raise ValueError("SGD_mode not valid. Acceptable values are: 'sgd', 'adagrad', 'rmsprop', 'adam'. Provided value was '{}'".format(
                sgd_mode))
        indptr = indices = None
        if profiles is not None:
            m = profiles.tocsr()
            if m.shape != (self.num_users, self.num_items):
                raise ValueError("slim_bpr_init: profiles must be %d x %d, given %r" % (self.num_users, self.num_items, m.shape))
            indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        L.check(self.lib.ganmf_slim_bpr_init(self.h, int(bool(symmetric)), L.SLIM_SGD_MODES[sgd_mode], float(learning_rate), float(lambda_i),
                                             float(lambda_j), float(gamma), float(beta_1), float(beta_2), int(seed) & (2 ** 64 - 1),
                                             indptr.ctypes.data_as(C.POINTER(C.c_int64)) if indptr is not None else None,
                                             _i32p(indices) if indices is not None else None), "ganmf_slim_bpr_init")

    def slim_bpr_draw(self, epoch, n_epochs=1):
        """(users, pos, neg), int32 [n_epochs * (num_users + 1)]: the samples of the epochs [epoch, epoch + n_epochs)"""
        n = int(n_epochs) * (self.num_users + 1)
        out = [np.zeros(n, dtype=np.int32) for _ in range(3)]
        L.check(self.lib.ganmf_slim_bpr_draw(self.h, int(epoch), int(n_epochs), _i32p(out[0]), _i32p(out[1]), _i32p(out[2])),
                "ganmf_slim_bpr_draw")
        return tuple(out)

    def slim_bpr_run(self, users, pos, neg, mode=L.SLIM_AUTO):
        """Applies the samples in list order (ganmf_slim_bpr_run); returns the number of levels (0 on the sequential route)."""
        u, i, j = (np.ascontiguousarray(v, dtype=np.int32).ravel() for v in (users, pos, neg))
        assert u.size == i.size == j.size
        levels = C.c_int64(0)
        L.check(self.lib.ganmf_slim_bpr_run(self.h, _i32p(u), _i32p(i), _i32p(j), u.size, int(mode), C.byref(levels)), "ganmf_slim_bpr_run")
        return int(levels.value)

    def slim_bpr_epochs(self, n_epochs=1, mode=L.SLIM_AUTO):
        """Draws and applies the next n_epochs epochs (ganmf_slim_bpr_epochs); returns the number of levels."""
        levels = C.c_int64(0)
        L.check(self.lib.ganmf_slim_bpr_epochs(self.h, int(n_epochs), int(mode), C.byref(levels)), "ganmf_slim_bpr_epochs")
        return int(levels.value)

    def slim_bpr_finish(self, topk):
        """get_S and the column top-K: the held W from the current S (ganmf_slim_bpr_finish); returns the stored weights."""
        nnz = C.c_int64(0)
        L.check(self.lib.ganmf_slim_bpr_finish(self.h, int(topk), C.byref(nnz)), "ganmf_slim_bpr_finish")
        self._knn_nnz = int(nnz.value)
        return self._knn_nnz

    def slim_bpr_state(self):
        """dict: S [num_items, num_items] float64 (dense, both halves when symmetric), state0 / state1 [num_items], beta_powers [2],
        epoch (ganmf_slim_bpr_get_state)"""
        n = self.num_items
        S = np.zeros((n, n), dtype=np.float64)
        s0, s1, pw = np.zeros(n), np.zeros(n), np.zeros(2)
        epoch = C.c_int64(0)
        L.check(self.lib.ganmf_slim_bpr_get_state(self.h, _f64p(S), _f64p(s0), _f64p(s1), _f64p(pw), C.byref(epoch)),
                "ganmf_slim_bpr_get_state")
        return {"S": S, "state0": s0, "state1": s1, "beta_powers": pw, "epoch": int(epoch.value)}

    # -- MF-BPR / FunkSVD (ganmf_mf_sgd_*, a MODEL_MF engine) ---------------------------------------
    def mf_sgd_init(self, algorithm, profiles, user_factors, item_factors, use_bias=False, sgd_mode="sgd", learning_rate=1e-3,
                    user_reg=0.0, item_reg=0.0, positive_reg=0.0, negative_reg=0.0, bias_reg=0.0, negative_interactions_quota=0.0, seed=0):
        """The float64 training state on the device (ganmf_mf_sgd_init).  profiles: the users x items CSR the samples are drawn from,
        with its stored values (canonical form).  The engine has num_factors + 2 columns when use_bias.  The rates are passed on as
        given: the caller rounds them."""
        if algorithm not in L.MF_SGD_ALGORITHMS:
            raise ValueError("Value for 'algorithm_name' not recognized. Acceptable values are {}, provided was '{}'".format(
                list(L.MF_SGD_ALGORITHMS), algorithm))
        if sgd_mode not in L.SLIM_SGD_MODES:
            raise ValueError("Value for 'sgd_mode' not recognized. Acceptable values are {}, provided was '{}'".format(
                ["sgd", "adam", "adagrad", "rmsprop"], sgd_mode))
        m = profiles.tocsr()
        if m.shape != (self.num_users, self.num_items):
            raise ValueError("mf_sgd_init: profiles must be %d x %d, given %r" % (self.num_users, self.num_items, m.shape))
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        data = np.ascontiguousarray(m.data, dtype=np.float64)
        U = np.ascontiguousarray(user_factors, dtype=np.float64)
        V = np.ascontiguousarray(item_factors, dtype=np.float64)
        k = self.cfg.num_factors - 2 * int(bool(use_bias))
        if U.shape != (self.num_users, k) or V.shape != (self.num_items, k):
            raise ValueError("mf_sgd_init: the initial factors must be %d x %d and %d x %d, given %r and %r" % (
                self.num_users, k, self.num_items, k, U.shape, V.shape))
        L.check(self.lib.ganmf_mf_sgd_init(self.h, L.MF_SGD_ALGORITHMS[algorithm], int(bool(use_bias)), L.SLIM_SGD_MODES[sgd_mode],
                                           float(learning_rate), float(user_reg), float(item_reg), float(positive_reg), float(negative_reg),
                                           float(bias_reg), float(negative_interactions_quota), int(seed) & (2 ** 64 - 1),
                                           indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices), _f64p(data), _f64p(U), _f64p(V)),
                "ganmf_mf_sgd_init")
        self._mf_sgd_info = (algorithm, k, bool(use_bias), int(indptr[-1]))

    @property
    def _mf_sgd(self):
        """(algorithm, num_factors, use_bias, nnz of the profiles) of the last mf_sgd_init; without one the library's own refusal"""
        if self._mf_sgd_info is None:
            L.check(self.lib.ganmf_mf_sgd_get_state(self.h, None, None, None, None, None), "ganmf_mf_sgd_get_state")
            raise L.GanmfError("ganmf_mf_sgd_init was not called through this Engine")
        return self._mf_sgd_info

    _mf_sgd_info = None

    def _mf_sgd_per_epoch(self, batch_size):
        algorithm, _, _, nnz = self._mf_sgd
        return ((self.num_users if algorithm == "MF_BPR" else nnz) // int(batch_size) + 1) * int(batch_size)

    def mf_sgd_draw(self, epoch, n_epochs=1, batch_size=1000):
        """(users, items, neg_items) int32 for MF_BPR, (users, items, ratings float64) for FUNK_SVD: the samples of the epochs
        [epoch, epoch + n_epochs) (ganmf_mf_sgd_draw)"""
        n = int(n_epochs) * self._mf_sgd_per_epoch(batch_size)
        bpr = self._mf_sgd[0] == "MF_BPR"
        users, items = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        third = np.zeros(n, dtype=np.int32 if bpr else np.float64)
        L.check(self.lib.ganmf_mf_sgd_draw(self.h, int(epoch), int(n_epochs), int(batch_size), _i32p(users), _i32p(items),
                                           _i32p(third) if bpr else None, None if bpr else _f64p(third)), "ganmf_mf_sgd_draw")
        return users, items, third

    def mf_sgd_run(self, users, items, third, batch_size, route=L.MF_SGD_AUTO):
        """Applies the samples in mini-batches of batch_size, in list order (ganmf_mf_sgd_run); `third` is neg_items for MF_BPR and
        the ratings for FUNK_SVD.  Returns the largest level count of a batch (0 on the sequential route)."""
        bpr = self._mf_sgd[0] == "MF_BPR"
        u, i = (np.ascontiguousarray(v, dtype=np.int32).ravel() for v in (users, items))
        t = np.ascontiguousarray(third, dtype=np.int32 if bpr else np.float64).ravel()
        assert u.size == i.size == t.size
        levels = C.c_int64(0)
        L.check(self.lib.ganmf_mf_sgd_run(self.h, _i32p(u), _i32p(i), _i32p(t) if bpr else None, None if bpr else _f64p(t), u.size,
                                          int(batch_size), int(route), C.byref(levels)), "ganmf_mf_sgd_run")
        return int(levels.value)

    def mf_sgd_epochs(self, n_epochs=1, batch_size=1000, route=L.MF_SGD_AUTO):
        """Draws and applies the next n_epochs epochs (ganmf_mf_sgd_epochs); returns the largest level count of a batch."""
        levels = C.c_int64(0)
        L.check(self.lib.ganmf_mf_sgd_epochs(self.h, int(n_epochs), int(batch_size), int(route), C.byref(levels)), "ganmf_mf_sgd_epochs")
        return int(levels.value)

    def mf_sgd_publish(self):
        """the float64 state rounded into the factor tensors, the biases as two more columns (ganmf_mf_sgd_publish)"""
        L.check(self.lib.ganmf_mf_sgd_publish(self.h), "ganmf_mf_sgd_publish")

    def _mf_sgd_split(self, block):
        _, k, _, _ = self._mf_sgd
        U, N = self.num_users, self.num_items
        a, b, c, d = U * k, U * k + N * k, U * k + N * k + U, U * k + N * k + U + N
        return {"USER_factors": block[:a].reshape(U, k), "ITEM_factors": block[a:b].reshape(N, k), "USER_bias": block[b:c],
                "ITEM_bias": block[c:d], "GLOBAL_bias": block[d:d + 1]}

    def mf_sgd_state(self):
        """dict: params / state0 / state1, each a dict of float64 USER_factors, ITEM_factors, USER_bias, ITEM_bias, GLOBAL_bias [1];
        beta_powers [2]; epoch (ganmf_mf_sgd_get_state)"""
        _, k, _, _ = self._mf_sgd
        size = (self.num_users + self.num_items) * (k + 1) + 1
        blocks = [np.zeros(size, dtype=np.float64) for _ in range(3)]
        pw, epoch = np.zeros(2), C.c_int64(0)
        L.check(self.lib.ganmf_mf_sgd_get_state(self.h, _f64p(blocks[0]), _f64p(blocks[1]), _f64p(blocks[2]), _f64p(pw), C.byref(epoch)),
                "ganmf_mf_sgd_get_state")
        return {"params": self._mf_sgd_split(blocks[0]), "state0": self._mf_sgd_split(blocks[1]), "state1": self._mf_sgd_split(blocks[2]),
                "beta_powers": pw, "epoch": int(epoch.value)}

    def mf_sgd_set_state(self, params=None, state0=None, state1=None, beta_powers=None, epoch=-1):
        """the reverse of mf_sgd_state: each of params / state0 / state1 a dict with all five members, or None to keep the block"""
        def join(d):
            if d is None:
                return None
            flat = np.concatenate([np.asarray(d[n], dtype=np.float64).ravel() for n in
                                   ("USER_factors", "ITEM_factors", "USER_bias", "ITEM_bias", "GLOBAL_bias")])
            _, k, _, _ = self._mf_sgd
            if flat.size != (self.num_users + self.num_items) * (k + 1) + 1:
                raise ValueError("mf_sgd_set_state: a block has %d values" % flat.size)
            return np.ascontiguousarray(flat)
        blocks = [join(d) for d in (params, state0, state1)]
        pw = None if beta_powers is None else np.ascontiguousarray(beta_powers, dtype=np.float64)
        L.check(self.lib.ganmf_mf_sgd_set_state(self.h, *[_f64p(b) if b is not None else None for b in blocks],
                                                _f64p(pw) if pw is not None else None, int(epoch)), "ganmf_mf_sgd_set_state")

    # -- CFGAN (ganmf_cfgan_*, a MODEL_CFGAN engine) ------------------------------------------------
    def cfgan_init(self, g_nodes, g_layers, g_act, d_batch, g_batch, scheme, zr_coefficient, seed, k_rows):
        """The generator, the two batch sizes, the scheme ("ZR" | "PM" | "ZP"), the zero-reconstruction coefficient, the mask
        sampler's seed and the subset size of every row (ganmf_cfgan_init); once per engine."""
        k = np.ascontiguousarray(k_rows, dtype=np.int32).ravel()
        assert k.size == self.num_users
        self._cfgan_batches = (min(int(d_batch), self.num_users), min(int(g_batch), self.num_users))
        L.check(self.lib.ganmf_cfgan_init(self.h, int(g_nodes), int(g_layers), L.ACT[g_act], int(d_batch), int(g_batch),
                                          L.CFGAN_SCHEMES[scheme], float(zr_coefficient), int(seed) & (2 ** 64 - 1), _i32p(k)),
                "ganmf_cfgan_init")

    @property
    def cfgan_words(self):
        """32-bit words per row of a mask plane"""
        return (self.num_items + 31) // 32

    def cfgan_draw_masks(self, epoch):
        """the device sampler's masks of `epoch` (ganmf_cfgan_draw_masks)"""
        L.check(self.lib.ganmf_cfgan_draw_masks(self.h, int(epoch)), "ganmf_cfgan_draw_masks")

    def cfgan_set_masks(self, zr=None, pm=None):
        """Uploads the two bit planes, uint32 [num_users, cfgan_words] each (pack_mask_rows' layout); None clears a plane."""
        planes = []
        for a in (zr, pm):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint32)
                assert a.shape == (self.num_users, self.cfgan_words)
            planes.append(a)
        u32p = C.POINTER(C.c_uint32)
        L.check(self.lib.ganmf_cfgan_set_masks(self.h, *[a.ctypes.data_as(u32p) if a is not None else None for a in planes]),
                "ganmf_cfgan_set_masks")

    def cfgan_masks(self):
        """(zr, pm): the two bit planes held, uint32 [num_users, cfgan_words] each (ganmf_cfgan_get_masks)"""
        out = [np.zeros((self.num_users, self.cfgan_words), dtype=np.uint32) for _ in range(2)]
        u32p = C.POINTER(C.c_uint32)
        L.check(self.lib.ganmf_cfgan_get_masks(self.h, out[0].ctypes.data_as(u32p), out[1].ctypes.data_as(u32p)), "ganmf_cfgan_get_masks")
        return out[0], out[1]

    def cfgan_step(self, kind, row0, nrows):
        """one optimiser step (0: D, 1: G) on the rows [row0, row0 + nrows); returns its loss (ganmf_cfgan_step)"""
        loss = C.c_float()
        L.check(self.lib.ganmf_cfgan_step(self.h, int(kind), int(row0), int(nrows), C.byref(loss)), "ganmf_cfgan_step")
        return np.float32(loss.value)

    def cfgan_epoch(self, epoch, d_steps=1, g_steps=1, draw=True):
        """One epoch in one call (ganmf_cfgan_epoch): the masks of `epoch` when draw, d_steps passes of D steps, g_steps passes of
        G steps.  Returns (d_losses, g_losses), one float32 per step."""
        db, gb = self._cfgan_batches
        nd, ng = int(d_steps) * (-(-self.num_users // db)), int(g_steps) * (-(-self.num_users // gb))
        dl, gl = np.zeros(max(nd, 1), dtype=np.float32), np.zeros(max(ng, 1), dtype=np.float32)
        L.check(self.lib.ganmf_cfgan_epoch(self.h, int(epoch), int(d_steps), int(g_steps), int(bool(draw)), _f32p(dl), _f32p(gl)),
                "ganmf_cfgan_epoch")
        return dl[:nd], gl[:ng]

    # -- CAAE (ganmf_caae_*, a MODEL_CAAE engine) --------------------------------------------------
    def caae_init(self, g_units, g_layers, d_bsize, m_batch, n_s, lmbda, beta, lr, seed, k_rows):
        """Both generators, the D slice length, the users and the policy draws per generator step, lmbda, beta, the learning rate, the
        samplers' seed and the size of every user's subset Nu (ganmf_caae_init); once per engine."""
        k = np.ascontiguousarray(k_rows, dtype=np.int32).ravel()
        assert k.size == self.num_users
        self._caae = (int(d_bsize), int(m_batch), int(n_s))
        L.check(self.lib.ganmf_caae_init(self.h, int(g_units), int(g_layers), int(d_bsize), int(m_batch), int(n_s), float(lmbda),
                                         float(beta), float(lr), int(seed) & (2 ** 64 - 1), _i32p(k)), "ganmf_caae_init")

    def caae_cdf(self, which, users=None, n=None):
        """(cdf [n, num_items], lse [n]) of generator `which` (0: G, 1: G') at its current parameters: of the listed users, or with
        users=None of all users -- refreshing the resident array the negatives are drawn from -- of which rows [0, n) come back."""
        if users is None:
            n = self.num_users if n is None else int(n)
            u = None
        else:
            u = np.ascontiguousarray(users, dtype=np.int32).ravel()
            n = u.size
        cdf, lse = np.zeros((n, self.num_items), dtype=np.float32), np.zeros(n, dtype=np.float32)
        L.check(self.lib.ganmf_caae_cdf(self.h, int(which), _i32p(u) if u is not None else None, n, _f32p(cdf), _f32p(lse)),
                "ganmf_caae_cdf")
        return cdf, lse

    def caae_draw_perm(self, epoch):
        """the order of the stored interactions for `epoch`: CSR position per position (ganmf_caae_draw_perm)"""
        out = np.zeros(max(self._nnz, 1), dtype=np.int32)
        L.check(self.lib.ganmf_caae_draw_perm(self.h, int(epoch), _i32p(out)), "ganmf_caae_draw_perm")
        return out[:self._nnz]

    def caae_draw_negatives(self, epoch, pass_, which):
        """one negative per position of the epoch's order from the resident CDF of generator `which` (ganmf_caae_draw_negatives)"""
        out = np.zeros(max(self._nnz, 1), dtype=np.int32)
        L.check(self.lib.ganmf_caae_draw_negatives(self.h, int(epoch), int(pass_), int(which), _i32p(out)), "ganmf_caae_draw_negatives")
        return out[:self._nnz]

    @property
    def caae_words(self):
        return (self.num_items + 31) // 32

    def caae_draw_batch(self, epoch, which, step):
        """(users [m], nu planes uint32 [m, words] (G; None for G'), items [m, n_s], cdf [m, num_items]) of a generator step's batch"""
        _, m, n_s = self._caae
        users, items = np.zeros(m, dtype=np.int32), np.zeros((m, n_s), dtype=np.int32)
        nu = np.zeros((m, self.caae_words), dtype=np.uint32)
        cdf = np.zeros((m, self.num_items), dtype=np.float32)
        L.check(self.lib.ganmf_caae_draw_batch(self.h, int(epoch), int(which), int(step), _i32p(users),
                                               nu.ctypes.data_as(C.POINTER(C.c_uint32)), _i32p(items), _f32p(cdf)), "ganmf_caae_draw_batch")
        return users, (nu if which == 0 else None), items, cdf

    def caae_draws(self, kind, index=0):
        """what the last caae_epoch drew: kind in _lib.CAAE_DRAWS, index = pass ("neg_*"), step ("users_*", "nu", "items_*") or user
        ("cdf_*": that row of the resident CDF)"""
        _, m, n_s = self._caae
        shape, dtype = {"perm": ((self._nnz,), np.int32), "neg_g": ((self._nnz,), np.int32), "neg_gpr": ((self._nnz,), np.int32),
                        "users_g": ((m,), np.int32), "users_gpr": ((m,), np.int32), "nu": ((m, self.caae_words), np.uint32),
                        "items_g": ((m, n_s), np.int32), "items_gpr": ((m, n_s), np.int32),
                        "cdf_g": ((self.num_items,), np.float32), "cdf_gpr": ((self.num_items,), np.float32)}[kind]
        out = np.zeros(shape, dtype=dtype)
        if out.size:
            L.check(self.lib.ganmf_caae_get_draws(self.h, L.CAAE_DRAWS[kind], int(index), out.ctypes.data_as(C.c_void_p), out.nbytes),
                    "ganmf_caae_get_draws")
        return out

    def caae_d_step(self, users, pos_items, neg_items):
        """one discriminator step on explicit triples; returns its loss (ganmf_caae_d_step)"""
        u, i, j = (np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (users, pos_items, neg_items))
        assert u.size == i.size == j.size
        loss = C.c_float()
        L.check(self.lib.ganmf_caae_d_step(self.h, _i32p(u), _i32p(i), _i32p(j), u.size, C.byref(loss)), "ganmf_caae_d_step")
        return np.float32(loss.value)

    def caae_g_step(self, which, users, nu, items):
        """one step of generator `which` on explicit users [m], Nu planes uint32 [m, words] (G only; None: empty) and policy items
        [m, n_s]; returns its loss (ganmf_caae_g_step)"""
        _, m, n_s = self._caae
        u = np.ascontiguousarray(users, dtype=np.int32).ravel()
        it = np.ascontiguousarray(items, dtype=np.int32).ravel()
        assert u.size == m and it.size == m * n_s
        p = None
        if nu is not None and which == 0:
            p = np.ascontiguousarray(nu, dtype=np.uint32)
            assert p.shape == (m, self.caae_words)
        loss = C.c_float()
        L.check(self.lib.ganmf_caae_g_step(self.h, int(which), _i32p(u), p.ctypes.data_as(C.POINTER(C.c_uint32)) if p is not None else None,
                                           _i32p(it), C.byref(loss)), "ganmf_caae_g_step")
        return np.float32(loss.value)

    def caae_epoch(self, epoch, d_steps=1, g_steps=1, gpr_steps=1):
        """One epoch in one call (ganmf_caae_epoch).  Returns (d_losses, g_losses, gpr_losses), one float32 per step."""
        d_bsize = self._caae[0]
        nd = int(d_steps) * 2 * (-(-self._nnz // d_bsize))
        dl, gl, pl = (np.zeros(max(n, 1), dtype=np.float32) for n in (nd, int(g_steps), int(gpr_steps)))
        L.check(self.lib.ganmf_caae_epoch(self.h, int(epoch), int(d_steps), int(g_steps), int(gpr_steps), _f32p(dl), _f32p(gl), _f32p(pl)),
                "ganmf_caae_epoch")
        return dl[:nd], gl[:int(g_steps)], pl[:int(gpr_steps)]

    def item_similarity(self):
        """The held item similarity matrix as the reference lays W_sparse out (ganmf_itemknn_get): scipy CSR float32
        [num_items, num_items], rows = neighbour, columns = item."""
        import scipy.sparse as sps
        n = self.num_items
        nnz = getattr(self, "_knn_nnz", None)
        if nnz is None:
            raise L.GanmfError("item_similarity: the engine holds no item similarity matrix")
        indptr = np.zeros(n + 1, dtype=np.int64)
        indices = np.zeros(max(nnz, 1), dtype=np.int32)
        data = np.zeros(max(nnz, 1), dtype=np.float32)
        L.check(self.lib.ganmf_itemknn_get(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices), _f32p(data)),
                "ganmf_itemknn_get")
        by_item = sps.csc_matrix((data[:nnz], indices[:nnz], indptr), shape=(n, n))      # column i = the neighbours of item i
        return by_item.tocsr()

    def set_item_similarity(self, W_sparse):
        """Uploads an item similarity matrix in the reference's layout (rows = neighbour, columns = item), any scipy format
        (ganmf_set_item_similarity)."""
        import scipy.sparse as sps
        W = sps.csc_matrix(W_sparse, dtype=np.float32)
        if W.shape != (self.num_items, self.num_items):
            raise ValueError("set_item_similarity: W_sparse must be %d x %d, given %r" % (self.num_items, self.num_items, W.shape))
        W.sum_duplicates()
        W.sort_indices()
        indptr = np.ascontiguousarray(W.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(W.indices, dtype=np.int32)
        data = np.ascontiguousarray(W.data, dtype=np.float32)
        L.check(self.lib.ganmf_set_item_similarity(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices), _f32p(data),
                                                   self.num_items), "ganmf_set_item_similarity")
        self._knn_nnz = int(indptr[-1])

    def user_similarity(self):
        """The held user similarity matrix as the reference lays W_sparse out (ganmf_userknn_get): scipy CSR float32
        [num_users, num_users], row u = the users whose profiles user u's scores sum, ascending."""
        import scipy.sparse as sps
        n = self.num_users
        nnz = getattr(self, "_knn_nnz", None)
        if nnz is None:
            raise L.GanmfError("user_similarity: the engine holds no user similarity matrix")
        indptr = np.zeros(n + 1, dtype=np.int64)
        indices = np.zeros(max(nnz, 1), dtype=np.int32)
        data = np.zeros(max(nnz, 1), dtype=np.float32)
        L.check(self.lib.ganmf_userknn_get(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices), _f32p(data)),
                "ganmf_userknn_get")
        return sps.csr_matrix((data[:nnz], indices[:nnz], indptr), shape=(n, n))

    def set_user_similarity(self, W_sparse):
        """Uploads a user similarity matrix in the reference's layout ([num_users, num_users], scores = W_sparse[users] . URM), any
        scipy format (ganmf_set_user_similarity): rows ascending, duplicates summed."""
        import scipy.sparse as sps
        W = sps.csr_matrix(W_sparse, dtype=np.float32)
        if W.shape != (self.num_users, self.num_users):
            raise ValueError("set_user_similarity: W_sparse must be %d x %d, given %r" % (self.num_users, self.num_users, W.shape))
        W.sum_duplicates()
        W.sort_indices()
        indptr = np.ascontiguousarray(W.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(W.indices, dtype=np.int32)
        data = np.ascontiguousarray(W.data, dtype=np.float32)
        L.check(self.lib.ganmf_set_user_similarity(self.h, indptr.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(indices), _f32p(data),
                                                   self.num_users), "ganmf_set_user_similarity")
        self._knn_nnz = int(indptr[-1])

    def snapshot_best(self):
        L.check(self.lib.ganmf_snapshot_best(self.h), "ganmf_snapshot_best")

    def restore_best(self):
        L.check(self.lib.ganmf_restore_best(self.h), "ganmf_restore_best")

    # -- measurement ------------------------------------------------------------------------
    def timer_start(self):
        """hipEvent on the library's stream in front of whatever is enqueued next (bench.py's timed region)."""
        L.check(self.lib.ganmf_stream_timer(self.h, 0, None), "ganmf_stream_timer")

    def timer_stop(self):
        """milliseconds the stream spent since timer_start (waits for the stream)."""
        ms = C.c_double(0.0)
        L.check(self.lib.ganmf_stream_timer(self.h, 1, C.byref(ms)), "ganmf_stream_timer")
        return float(ms.value)

    def profile(self, on):
        L.check(self.lib.ganmf_profile_enable(self.h, int(on)), "ganmf_profile_enable")

    def profile_read(self):
        buf = (L.ProfEntry * L.PROF_MAX)()
        n = C.c_int32()
        L.check(self.lib.ganmf_profile_read(self.h, buf, L.PROF_MAX, C.byref(n)), "ganmf_profile_read")
        return [dict(name=buf[i].name.decode(), launches=buf[i].launches, ms=buf[i].ms, flops=buf[i].flops,
                     bytes=buf[i].bytes) for i in range(n.value)]

    def bench_scores(self, n, transposed=False, iters=10):
        ms = C.c_float()
        L.check(self.lib.ganmf_bench_scores(self.h, n, int(transposed), iters, C.byref(ms)), "ganmf_bench_scores")
        return ms.value

    def comm_info(self):
        """(ranks in the communicator as RCCL reports them, this handle's rank); (0, -1) without a communicator"""
        w, r = C.c_int32(0), C.c_int32(-1)
        L.check(self.lib.ganmf_comm_info(self.h, C.byref(w), C.byref(r)), "ganmf_comm_info")
        return int(w.value), int(r.value)

    def comm_abort(self):
        """end this engine's communicator from ANOTHER thread than the one inside a training call (ganmf_comm_abort): the
        call in flight returns with an error instead of waiting for a peer that failed; close() is what is left to do"""
        if self.h:
            L.check(self.lib.ganmf_comm_abort(self.h), "ganmf_comm_abort")

    def comm_init_local(self, group_id):
        """join the in-process loopback communicator `group_id` (all world_size engines of this process must)"""
        L.check(self.lib.ganmf_comm_init_local(self.h, int(group_id)), "ganmf_comm_init_local")

    def comm_unique_id(self):
        """128 bytes rank 0 hands to every rank's comm_init (ganmf_comm_unique_id)"""
        return comm_unique_id()

    def comm_init(self, id_bytes):
        arr = (C.c_uint8 * 128).from_buffer_copy(bytes(id_bytes))
        L.check(self.lib.ganmf_comm_init(self.h, arr), "ganmf_comm_init")


def comm_unique_id():
    lib = L.load_library()
    arr = (C.c_uint8 * 128)()
    L.check(lib.ganmf_comm_unique_id(arr), "ganmf_comm_unique_id")
    return bytes(arr)


def gemm_f32(A, B, a_kmajor=False, b_kmajor=False, tile=0, nsplit=0, iters=1, device=0):
    """C = op(A).op(B) through the stand-alone entry (tests / bench)."""
    lib = L.load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    K, M = (A.shape if a_kmajor else A.shape[::-1])
    Kb, N = (B.shape if b_kmajor else B.shape[::-1])
    assert K == Kb, (A.shape, B.shape)
    out = np.empty((M, N), dtype=np.float32)
    ms = C.c_float()
    L.check(lib.ganmf_gemm_f32(device, _f32p(A), _f32p(B), _f32p(out), M, N, K, int(a_kmajor), int(b_kmajor),
                               tile, nsplit, iters, C.byref(ms)), "ganmf_gemm_f32")
    return out, ms.value


def gemm_f32_ex(A, B, a_kmajor=False, b_kmajor=False, tile=0, nsplit=0, iters=1, device=0, a_gather=None, bk=0, adam=False):
    """gemm_f32 with what only the step's launches use (ganmf_gemm_f32_ex): `a_gather` -- row r of the product's A is A[a_gather[r]];
    `bk` = 32 -- the 4-wave staged kernel's 32-deep K-tile; `adam` -- the fused-Adam epilogue on zero state: returns (theta, m, ms)
    with m = (1 - beta1) x the product (one launch: no timing, ms = 0)."""
    lib = L.load_library()
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    K, M = (A.shape if a_kmajor else A.shape[::-1])
    Kb, N = (B.shape if b_kmajor else B.shape[::-1])
    assert K == Kb, (A.shape, B.shape)
    ids, a_rows = None, 0
    if a_gather is not None:
        ids = np.ascontiguousarray(a_gather, dtype=np.int32)
        a_rows, M = A.shape[0], len(ids)
    out = np.empty((M, N), dtype=np.float32)
    mom = np.empty((M, N), dtype=np.float32) if adam else None
    ms = C.c_float()
    L.check(lib.ganmf_gemm_f32_ex(device, _f32p(A), _f32p(B), _f32p(out), M, N, K, int(a_kmajor), int(b_kmajor), tile, nsplit, iters,
                                  None if adam else C.byref(ms), ids.ctypes.data_as(C.POINTER(C.c_int32)) if ids is not None else None, a_rows, bk,
                                  _f32p(mom) if adam else None), "ganmf_gemm_f32_ex")
    return (out, mom, ms.value) if adam else (out, ms.value)
