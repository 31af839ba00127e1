"""ctypes binding of libganmf_hip.so — exactly the symbols include/ganmf_hip.h declares."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("GANMF_LIB_PATH") or os.path.join(_HERE, "libganmf_hip.so")      # (GANMF_LIB_PATH: A/B runs of two builds)
_lib = None

ABI_VERSION = 2
MODEL_GANMF, MODEL_DISGANMF, MODEL_MF, MODEL_ITEMSIM, MODEL_CFGAN, MODEL_CAAE = 0, 1, 2, 3, 4, 5
ITEMKNN_MAX_TOPK = 1024            # include/ganmf_hip.h GANMF_ITEMKNN_MAX_TOPK
# include/ganmf_hip.h GANMF_ITEMKNN_*: the denominator ganmf_itemknn_fit applies to the dot products
ITEMKNN_PRODUCT, ITEMKNN_TANIMOTO, ITEMKNN_DICE, ITEMKNN_TVERSKY, ITEMKNN_SHRINK_ONLY, ITEMKNN_RAW = 0, 1, 2, 3, 4, 5
# include/ganmf_hip.h GANMF_SLIM_*: the optimiser of ganmf_slim_bpr_init and the route of ganmf_slim_bpr_run
SLIM_SGD_MODES = {"sgd": 0, "adagrad": 1, "rmsprop": 2, "adam": 3}
SLIM_AUTO, SLIM_SEQUENTIAL, SLIM_LEVELLED = 0, 1, 2
# include/ganmf_hip.h GANMF_MF_SGD_*: the algorithm of ganmf_mf_sgd_init, the route of ganmf_mf_sgd_run and the two limits
MF_SGD_ALGORITHMS = {"MF_BPR": 0, "FUNK_SVD": 1}
MF_SGD_AUTO, MF_SGD_SEQUENTIAL, MF_SGD_LEVELLED = 0, 1, 2
MF_SGD_MAX_FACTORS, MF_SGD_MAX_BATCH = 1024, 1 << 20
ALS_MAX_FACTORS = 256              # include/ganmf_hip.h GANMF_ALS_MAX_FACTORS
SVD_MAX_RANDOM = 280               # include/ganmf_hip.h GANMF_SVD_MAX_RANDOM
NMF_MAX_FACTORS = 270              # include/ganmf_hip.h GANMF_NMF_MAX_FACTORS
NMF_FROBENIUS, NMF_KULLBACK_LEIBLER = 0, 1      # include/ganmf_hip.h GANMF_NMF_*: the beta_loss of ganmf_nmf_mu / ganmf_nmf_error
FLAG_MFMA_F32, FLAG_MFMA_BF16, FLAG_MFMA_F16 = 1, 2, 4     # include/ganmf_hip.h GANMF_FLAG_*
MFMA_FLAGS = {None: 0, "auto": 0, "f32": FLAG_MFMA_F32, "bf16": FLAG_MFMA_BF16, "f16": FLAG_MFMA_F16}
ACT = {"linear": 0, "tanh": 1, "relu": 2, "sigmoid": 3}
T_USER_EMB, T_ITEM_EMB = 100, 101
T_CFGAN_G0 = 200                  # include/ganmf_hip.h GANMF_T_CFGAN_G0: first generator tensor of a MODEL_CFGAN handle
CFGAN_SCHEMES = {"ZR": 0, "PM": 1, "ZP": 2}      # include/ganmf_hip.h GANMF_CFGAN_*
# include/ganmf_hip.h GANMF_T_CAAE_*: the item bias and the first tensor of G / G' of a MODEL_CAAE handle; GANMF_CAAE_*
T_CAAE_ITEM_BIAS, T_CAAE_G0, T_CAAE_GPR0 = 102, 300, 400
CAAE_MAX_FACTORS, CAAE_MAX_D_BSIZE = 256, 16384
CAAE_DRAWS = {"perm": 0, "neg_g": 1, "neg_gpr": 2, "users_g": 3, "users_gpr": 4, "nu": 5, "items_g": 6, "items_gpr": 7, "cdf_g": 8,
              "cdf_gpr": 9}
SLOT_PARAM, SLOT_ADAM_M, SLOT_ADAM_V, SLOT_BEST = 0, 1, 2, 3
EVAL_METRICS = ("ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "HIT_RATE", "ARHR")
EVAL_MAX_CUTOFFS = 8
EVAL_MAX_GROUPS = 256             # include/ganmf_hip.h GANMF_EVAL_MAX_GROUPS
# ganmf_evaluate_full's sums per cut-off (GANMF_EVAL_FULL_METRICS): NON_EMPTY = number of non-empty lists
EVAL_FULL_METRICS = EVAL_METRICS + ("RMSE", "NOVELTY", "AVERAGE_POPULARITY", "NON_EMPTY")
PROF_MAX = 80
RECOMMEND_MAX_CUTOFF = 1024        # include/ganmf_hip.h GANMF_RECOMMEND_MAX_CUTOFF
CANDIDATES_MAX_PER_ROW = 8192     # include/ganmf_hip.h GANMF_CANDIDATES_MAX_PER_ROW

# every exported symbol of include/ganmf_hip.h (checked by tests/test_abi.py)
SYMBOLS = [
    "ganmf_create", "ganmf_destroy", "ganmf_comm_unique_id", "ganmf_comm_init", "ganmf_comm_init_local", "ganmf_comm_abort", "ganmf_comm_info", "ganmf_set_urm_csr",
    "ganmf_set_tensor", "ganmf_get_tensor", "ganmf_tensor_shape", "ganmf_get_adam_powers",
    "ganmf_set_adam_powers", "ganmf_train_epoch", "ganmf_train_epoch_ragged", "ganmf_train_step", "ganmf_scores",
    "ganmf_set_seen_csr", "ganmf_set_score_filter", "ganmf_recommend", "ganmf_set_test_csr", "ganmf_evaluate", "ganmf_set_test_ratings", "ganmf_set_eval_item_weights", "ganmf_evaluate_full", "ganmf_set_candidates_csr", "ganmf_recommend_candidates", "ganmf_evaluate_candidates", "ganmf_evaluate_groups", "ganmf_set_items_to_ignore", "ganmf_set_item_diversity", "ganmf_evaluate_diversity", "ganmf_score_similarity", "ganmf_set_discriminate_block", "ganmf_discriminate", "ganmf_als_set_confidence", "ganmf_als_half_sweep", "ganmf_pure_svd", "ganmf_nmf_mu", "ganmf_nmf_cd", "ganmf_nmf_error", "ganmf_itemknn_fit", "ganmf_itemknn_get", "ganmf_set_item_similarity", "ganmf_userknn_fit", "ganmf_userknn_get", "ganmf_set_user_similarity", "ganmf_p3_fit", "ganmf_slim_bpr_init", "ganmf_slim_bpr_draw", "ganmf_slim_bpr_run", "ganmf_slim_bpr_epochs", "ganmf_slim_bpr_finish", "ganmf_slim_bpr_get_state", "ganmf_mf_sgd_init", "ganmf_mf_sgd_draw", "ganmf_mf_sgd_run", "ganmf_mf_sgd_epochs", "ganmf_mf_sgd_publish", "ganmf_mf_sgd_get_state", "ganmf_mf_sgd_set_state", "ganmf_cfgan_init", "ganmf_cfgan_draw_masks", "ganmf_cfgan_set_masks", "ganmf_cfgan_get_masks", "ganmf_cfgan_step", "ganmf_cfgan_epoch", "ganmf_caae_init", "ganmf_caae_cdf", "ganmf_caae_draw_perm", "ganmf_caae_draw_negatives", "ganmf_caae_draw_batch", "ganmf_caae_get_draws", "ganmf_caae_d_step", "ganmf_caae_g_step", "ganmf_caae_epoch", "ganmf_snapshot_best", "ganmf_restore_best", "ganmf_profile_enable", "ganmf_profile_read", "ganmf_stream_timer",
    "ganmf_bench_scores", "ganmf_gemm_f32", "ganmf_gemm_f32_ex", "ganmf_crc32c", "ganmf_device_count", "ganmf_live_device_bytes", "ganmf_abi_version", "ganmf_last_error",
]


class Cfg(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32),
        ("num_users", C.c_int64), ("num_items", C.c_int64),
        ("num_factors", C.c_int32), ("emb_dim", C.c_int32),
        ("d_layers", C.c_int32), ("d_act", C.c_int32), ("batch_size", C.c_int32),
        ("d_lr", C.c_float), ("g_lr", C.c_float), ("d_reg", C.c_float), ("g_reg", C.c_float),
        ("m", C.c_float), ("recon_coefficient", C.c_float),
        ("device", C.c_int32), ("world_size", C.c_int32), ("rank", C.c_int32),
        ("row_offset", C.c_int64), ("flags", C.c_uint32),
    ]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


def library_path():
    return _LIB_PATH


def build_library(verbose=False):
    """hipcc --offload-arch=gfx950 build of the in-tree shared library (no GPU needed)."""
    res = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise RuntimeError("building libganmf_hip.so failed")
    return _LIB_PATH


def load_library():
    """Loads libganmf_hip.so or raises: the HIP path is the only path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            "libganmf_hip.so is missing (%s). Build it with `make -C ganmf_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % _LIB_PATH)
    lib = C.CDLL(_LIB_PATH)
    P = C.POINTER
    vp, i32, i64, f32p = C.c_void_p, C.c_int32, C.c_int64, P(C.c_float)
    sig = {
        "ganmf_create": (C.c_int, [P(Cfg), P(vp)]),
        "ganmf_destroy": (C.c_int, [vp]),
        "ganmf_comm_unique_id": (C.c_int, [P(C.c_uint8)]),
        "ganmf_comm_init": (C.c_int, [vp, P(C.c_uint8)]),
        "ganmf_comm_init_local": (C.c_int, [vp, i32]),
        "ganmf_comm_abort": (C.c_int, [vp]),
        "ganmf_comm_info": (C.c_int, [vp, P(i32), P(i32)]),
        "ganmf_set_urm_csr": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), f32p, i64, i64]),
        "ganmf_set_tensor": (C.c_int, [vp, C.c_int, C.c_int, f32p, i64]),
        "ganmf_get_tensor": (C.c_int, [vp, C.c_int, C.c_int, f32p, i64]),
        "ganmf_tensor_shape": (C.c_int, [vp, C.c_int, P(C.c_int64), P(C.c_int64)]),
        "ganmf_get_adam_powers": (C.c_int, [vp, f32p]),
        "ganmf_set_adam_powers": (C.c_int, [vp, f32p]),
        "ganmf_train_epoch": (C.c_int, [vp, P(C.c_int32), i64, i32, i32, i64, P(C.c_int32), f32p, f32p]),
        "ganmf_train_epoch_ragged": (C.c_int, [vp, P(C.c_int32), i64, i32, i32, i64, P(C.c_int32), P(C.c_int32), f32p, f32p]),
        "ganmf_train_step": (C.c_int, [vp, C.c_int, P(C.c_int32), i32, f32p]),
        "ganmf_scores": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, f32p]),
        "ganmf_set_seen_csr": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), i64, i64]),
        "ganmf_set_score_filter": (C.c_int, [vp, P(C.c_int32), i64, C.c_int]),
        "ganmf_recommend": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, i32, C.c_int, P(C.c_int32), f32p]),
        "ganmf_set_test_csr": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), P(C.c_double), i64, i64]),
        "ganmf_evaluate": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, C.c_int, P(C.c_int32), i32, P(C.c_double), P(C.c_double),
                                     P(C.c_double)]),
        "ganmf_set_test_ratings": (C.c_int, [vp, f32p, i64]),
        "ganmf_set_eval_item_weights": (C.c_int, [vp, P(C.c_double), P(C.c_double), i64]),
        "ganmf_evaluate_full": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, C.c_int, P(C.c_int32), i32, P(C.c_double),
                                          P(C.c_double), P(C.c_double), P(C.c_int64)]),
        "ganmf_set_candidates_csr": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), i64, i64]),
        "ganmf_recommend_candidates": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, i32, C.c_int, P(C.c_int32), f32p]),
        "ganmf_evaluate_candidates": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, C.c_int, P(C.c_int32), i32, P(C.c_double),
                                                P(C.c_double), P(C.c_double), P(C.c_int64)]),
        "ganmf_evaluate_groups": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, C.c_int, C.c_int, P(C.c_int32), i32, P(C.c_double),
                                            P(C.c_double), P(C.c_int32), i32, P(C.c_double), P(C.c_int64), P(C.c_double)]),
        "ganmf_set_items_to_ignore": (C.c_int, [vp, P(C.c_int32), i64]),
        "ganmf_set_item_diversity": (C.c_int, [vp, f32p, i64]),
        "ganmf_evaluate_diversity": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, C.c_int, C.c_int, P(C.c_int32), i32, P(C.c_double),
                                               P(C.c_double)]),
        "ganmf_score_similarity": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, i32, P(C.c_double), f32p, f32p]),
        "ganmf_set_discriminate_block": (C.c_int, [vp, i64]),
        "ganmf_discriminate": (C.c_int, [vp, P(C.c_int32), i64, C.c_int, f32p, P(C.c_double)]),
        "ganmf_als_set_confidence": (C.c_int, [vp, C.c_int, P(C.c_int64), P(C.c_int32), f32p, i64, i64]),
        "ganmf_als_half_sweep": (C.c_int, [vp, C.c_int, C.c_float]),
        "ganmf_pure_svd": (C.c_int, [vp, f32p, C.c_int, C.c_int, f32p]),
        "ganmf_nmf_mu": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, P(C.c_double)]),
        "ganmf_nmf_cd": (C.c_int, [vp, P(C.c_int32), C.c_int, C.c_int, P(C.c_double)]),
        "ganmf_nmf_error": (C.c_int, [vp, C.c_int, P(C.c_double)]),
        "ganmf_itemknn_fit": (C.c_int, [vp, C.c_int, i32, C.c_float, C.c_float, C.c_float, f32p, f32p, P(C.c_int64)]),
        "ganmf_itemknn_get": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), f32p]),
        "ganmf_set_item_similarity": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), f32p, i64]),
        "ganmf_userknn_fit": (C.c_int, [vp, C.c_int, i32, C.c_float, C.c_float, C.c_float, f32p, f32p, P(C.c_int64)]),
        "ganmf_userknn_get": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), f32p]),
        "ganmf_set_user_similarity": (C.c_int, [vp, P(C.c_int64), P(C.c_int32), f32p, i64]),
        "ganmf_p3_fit": (C.c_int, [vp, i32, i32, C.c_int, f32p, f32p, P(C.c_int64)]),
        "ganmf_slim_bpr_init": (C.c_int, [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_uint64, P(C.c_int64), P(C.c_int32)]),
        "ganmf_slim_bpr_draw": (C.c_int, [vp, i64, i64, P(C.c_int32), P(C.c_int32), P(C.c_int32)]),
        "ganmf_slim_bpr_run": (C.c_int, [vp, P(C.c_int32), P(C.c_int32), P(C.c_int32), i64, C.c_int, P(C.c_int64)]),
        "ganmf_slim_bpr_epochs": (C.c_int, [vp, i64, C.c_int, P(C.c_int64)]),
        "ganmf_slim_bpr_finish": (C.c_int, [vp, i32, P(C.c_int64)]),
        "ganmf_slim_bpr_get_state": (C.c_int, [vp, P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_int64)]),
        "ganmf_mf_sgd_init": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                        C.c_double, C.c_uint64, P(C.c_int64), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double)]),
        "ganmf_mf_sgd_draw": (C.c_int, [vp, i64, i64, i64, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_double)]),
        "ganmf_mf_sgd_run": (C.c_int, [vp, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_double), i64, i64, C.c_int, P(C.c_int64)]),
        "ganmf_mf_sgd_epochs": (C.c_int, [vp, i64, i64, C.c_int, P(C.c_int64)]),
        "ganmf_mf_sgd_publish": (C.c_int, [vp]),
        "ganmf_mf_sgd_get_state": (C.c_int, [vp, P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_int64)]),
        "ganmf_mf_sgd_set_state": (C.c_int, [vp, P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double), i64]),
        "ganmf_cfgan_init": (C.c_int, [vp, i32, i32, C.c_int, i32, i32, C.c_int, C.c_float, C.c_uint64, P(C.c_int32)]),
        "ganmf_cfgan_draw_masks": (C.c_int, [vp, i64]),
        "ganmf_cfgan_set_masks": (C.c_int, [vp, P(C.c_uint32), P(C.c_uint32)]),
        "ganmf_cfgan_get_masks": (C.c_int, [vp, P(C.c_uint32), P(C.c_uint32)]),
        "ganmf_cfgan_step": (C.c_int, [vp, C.c_int, i64, i32, f32p]),
        "ganmf_cfgan_epoch": (C.c_int, [vp, i64, i32, i32, C.c_int, f32p, f32p]),
        "ganmf_caae_init": (C.c_int, [vp, i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_uint64, P(C.c_int32)]),
        "ganmf_caae_cdf": (C.c_int, [vp, C.c_int, P(C.c_int32), i32, f32p, f32p]),
        "ganmf_caae_draw_perm": (C.c_int, [vp, i64, P(C.c_int32)]),
        "ganmf_caae_draw_negatives": (C.c_int, [vp, i64, i32, C.c_int, P(C.c_int32)]),
        "ganmf_caae_draw_batch": (C.c_int, [vp, i64, C.c_int, i32, P(C.c_int32), P(C.c_uint32), P(C.c_int32), f32p]),
        "ganmf_caae_get_draws": (C.c_int, [vp, C.c_int, i32, vp, i64]),
        "ganmf_caae_d_step": (C.c_int, [vp, P(C.c_int32), P(C.c_int32), P(C.c_int32), i32, f32p]),
        "ganmf_caae_g_step": (C.c_int, [vp, C.c_int, P(C.c_int32), P(C.c_uint32), P(C.c_int32), f32p]),
        "ganmf_caae_epoch": (C.c_int, [vp, i64, i32, i32, i32, f32p, f32p, f32p]),
        "ganmf_crc32c": (C.c_uint32, [C.c_uint32, vp, C.c_uint64]),
        "ganmf_snapshot_best": (C.c_int, [vp]),
        "ganmf_restore_best": (C.c_int, [vp]),
        "ganmf_profile_enable": (C.c_int, [vp, C.c_int]),
        "ganmf_profile_read": (C.c_int, [vp, P(ProfEntry), i32, P(i32)]),
        "ganmf_stream_timer": (C.c_int, [vp, C.c_int, P(C.c_double)]),
        "ganmf_bench_scores": (C.c_int, [vp, i64, C.c_int, i32, f32p]),
        "ganmf_gemm_f32": (C.c_int, [C.c_int, f32p, f32p, f32p, i64, i64, i64, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, f32p]),
        "ganmf_gemm_f32_ex": (C.c_int, [C.c_int, f32p, f32p, f32p, i64, i64, i64, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, f32p, P(C.c_int32), i64, C.c_int, f32p]),
        "ganmf_device_count": (C.c_int, []),
        "ganmf_live_device_bytes": (i64, []),
        "ganmf_abi_version": (C.c_int, []),
        "ganmf_last_error": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.ganmf_abi_version() != ABI_VERSION:
        raise RuntimeError("libganmf_hip.so ABI %d != binding %d" % (lib.ganmf_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


class GanmfError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        msg = load_library().ganmf_last_error()
        text = "%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?")
        if b"out of memory" in (msg or b"").lower():
            raise MemoryError(text)
        raise GanmfError(text)
