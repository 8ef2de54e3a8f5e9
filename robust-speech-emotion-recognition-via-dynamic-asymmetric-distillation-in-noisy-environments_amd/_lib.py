"""ctypes binding of the C ABI in include/dad.h (libdad_hip.so).

The structures below mirror dad.h field for field.  Loading fails loudly: there is no
Python or PyTorch fallback for any operator of the step.
"""
import ctypes
import os

from . import _build

c_float_p = ctypes.POINTER(ctypes.c_float)

DAD_ABI_VERSION = 10       # dad.h DAD_ABI_VERSION this binding mirrors
DAD_NPARAM = 256 * 768 + 256 + 4 * 256 + 4
DAD_GRAD_EXTRA = 16
DAD_GRAD_FLOATS = DAD_NPARAM + DAD_GRAD_EXTRA
DAD_DACP_FLOATS = 20
DAD_TAIL_HDR = 64
DAD_MAX_BATCH = 1024
PREC_FP32, PREC_BF16, PREC_FP16 = 0, 1, 2
DRAW_WEAK, DRAW_STRONG, DRAW_FEAT_KEEP, DRAW_TSTART, DRAW_KEEP1, DRAW_KEEP2 = range(1, 7)
RNG_EXPLICIT, RNG_COUNTER = 0, 1
PREP_CLEAN, PREP_NOISY = 1, 2     # dad.h DAD_PREP_* (dad_step_backward_ahead_split / dad_step_prepare_rows)
STEP_LAUNCHES = 6                 # dad.h DAD_STEP_LAUNCHES (dad_step_plan_kernels): prep, encode, pool, tail, wgrad, reduce
STORE_F32, STORE_F16, STORE_BF16 = 0, 1, 2   # dad.h DAD_STORE_* (dad_collate, dad_batch.xc_dtype / xn_dtype)
E_ARG, E_SHAPE, E_COMM, E_UNSUPPORTED = 1001, 1002, 1003, 1004   # dad.h DAD_E_*

# tail header slots (dad.h DAD_T_*)
T_TOTAL, T_CE, T_KL, T_ECDA, T_SCL, T_MSUM, T_CLIPNORM, T_CLIPCOEF = range(8)
T_W, T_TAU_BEFORE, T_TAU_AFTER, T_FLOORED, T_ECDA_TERM, T_ECDA_GATE = 8, 12, 16, 20, 24, 28
T_KL_ON, T_ECDA_ON, T_RANGE, T_TAU_HAT = 32, 33, 34, 40
RANGE_NONFINITE, RANGE_POOL_TIMEOUT = 1, 2   # bits of the T_RANGE word (dad.h DAD_RANGE_*)
TRACE_HDR_WORDS, TRACE_REC_WORDS, TRACE_MASKED_IN = 4, 4, 0x100   # dad.h DAD_TRACE_* (dad_trace_append)

# result block of dad_cluster_metrics (dad.h DAD_CM_*): float64 slots
CM_SILHOUETTE, CM_CH, CM_VALID, CM_M, CM_K, CM_COUNTS, CM_SIL_CLASS, CM_W, CM_B, CM_NONFINITE = 0, 1, 2, 3, 4, 5, 9, 13, 14, 15
CM_SLOTS, CM_MAX_N, CM_TILE, CM_MAX_CHUNKS = 16, 65536, 64, 16

# dad_tsne_* (dad.h DAD_TS_*): float64 slots of the out block, limits, the workspace word of the non-finite count
TS_Z, TS_KL, TS_GRAD_NORM, TS_N_ITER, TS_N_CHECKS, TS_SLOTS = 0, 1, 2, 3, 4, 8
TS_MAX_N, TS_TILE, TS_MAX_CHUNKS, TS_WS_NONFINITE = 16384, 64, 32, 0

# result block of dad_domain_gap (dad.h DAD_DG_*): float64 slots ([4] per class from DG_C_GATE on), limits
DG_VALID, DG_N_SRC, DG_N_TGT, DG_NONFINITE, DG_REPULSION, DG_ECDA_LOSS, DG_MMD_CLASS_MEAN = range(7)
DG_G_GATE, DG_G_BANDWIDTH, DG_G_SS, DG_G_TT, DG_G_ST, DG_G_MMD = range(8, 14)
(DG_C_GATE, DG_C_BANDWIDTH, DG_C_SS, DG_C_TT, DG_C_ST, DG_C_MMD, DG_C_N_SRC, DG_C_N_TGT, DG_C_W_TGT,
 DG_C_COMPACTNESS, DG_C_SHIFT, DG_C_ATTENTION) = range(16, 64, 4)
DG_SLOTS, DG_MAX_N, DG_TILE, DG_MAX_CHUNKS = 64, 65536, 64, 16

# dad_knn / dad_knn_vote / dad_trustworthiness (dad.h DAD_KNN_*, DAD_KV_*, DAD_TW_*): modes and limits, the workspace
# word of the non-finite count, the int64 slots of the vote's block, the float64 slots of the trustworthiness block
KNN_ALL, KNN_SAME, KNN_OTHER = 0, 1, 2
KNN_MAX_K, KNN_MAX_N, KNN_TILE, KNN_MAX_CHUNKS, KNN_WS_NONFINITE = 32, 65536, 64, 16, 0
KV_CONFUSION, KV_QUERIES, KV_NO_VOTE, KV_SLOTS = 0, 32, 34, 40
TW_T, TW_PENALTY, TW_N, TW_K, TW_VALID, TW_NONFINITE, TW_SLOTS = 0, 1, 2, 3, 4, 5, 8

# result block of dad_scl (dad.h DAD_SCL_*): float32 slots ([4] anchors per class from SCL_ANCHORS on), limits
SCL_LOSS, SCL_V, SCL_MEMBERS, SCL_ANCHORS, SCL_NONFINITE, SCL_SLOTS = 0, 1, 2, 3, 7, 8
SCL_MAX_N, SCL_TILE, SCL_MAX_CHUNKS = 2048, 64, 8


def ts_ld(n):
    """dad.h DAD_TS_LD: the row stride of P."""
    return (n + TS_TILE - 1) // TS_TILE * TS_TILE


def tail_floats(bn):
    return DAD_TAIL_HDR + bn * 7


# result block of dad_eval_split (dad.h DAD_EV_*): int64 counts, then float64 moments [4][3]
EV_CONF_STUDENT, EV_CONF_TEACHER, EV_DISAGREE, EV_N, EV_N_LABELLED, EV_N_SKIPPED, EV_N_NONFINITE = 0, 16, 32, 33, 34, 35, 36
EV_COUNTS = 40
EV_MOMENTS, EV_M_COUNT, EV_M_MEAN, EV_M_VAR = 3, 0, 1, 2

# dad_eval_windows (dad.h DAD_WIN_*, DAD_EW_*): modes, the int64 slots of the result block
WIN_SLIDING, WIN_PREFIX = 0, 1
EW_CONF_MEAN, EW_CONF_VOTE, EW_CONF_LAST = 0, 16, 32
EW_N, EW_N_LABELLED, EW_N_EMPTY, EW_N_WINDOWS, EW_N_NONFINITE = 48, 49, 50, 51, 52
EW_SETTLE_SUM, EW_SWITCHES_SUM, EW_SETTLE_FRAMES_SUM = 53, 54, 55
EW_CURVE, EW_REACHED, EW_CORRECT, EW_CARRIED, EW_SLOTS = 64, 64, 128, 192, 256

# dad_eval_noise (dad.h DAD_EN_*): the level limit, the int64 slots of the counts block, the float64 slots of the sums
EN_MAX_LEVELS = 8
EN_CONF, EN_FLIPS, EN_SURVIVE = 0, 128, 136
EN_N, EN_N_LABELLED, EN_N_SKIPPED, EN_N_NONFINITE, EN_LEVELS, EN_COUNTS = 144, 145, 146, 147, 148, 160
EN_SUM_SCORE, EN_SUM_DRIFT, EN_SUM_KL, EN_SUMS = 0, 8, 16, 24
# dad_eval_models (dad.h DAD_EM_*): the model limit, the members (K models, the mean ensemble at K, the vote at K + 1),
# the int64 slots of the counts block and the float64 slots of the sums ([quantity][member])
EM_MAX_MODELS, EM_MEMBERS = 8, 10
EM_CONF, EM_DISAGREE, EM_ONLY, EM_HIST = 0, 160, 260, 360
EM_N, EM_N_LABELLED, EM_N_SKIPPED, EM_NONFINITE, EM_K, EM_COUNTS = 369, 370, 371, 372, 380, 384
EM_SUM_SCORE, EM_SUM_ENTROPY, EM_SUM_NLL, EM_SUM_BRIER, EM_SUMS = 0, 10, 20, 30, 40

# dad_input_grad (dad.h DAD_IG_*): the int64 slots of the counts block
IG_FRAMES, IG_NONFINITE, IG_ZERO, IG_COUNTS = 0, 1, 2, 4

# dad_attribution (dad.h DAD_AT_*): the int64 slots of the counts block, and dad_attribution_plan's slots
AT_FRAMES, AT_NONFINITE, AT_CROSS, AT_ONE, AT_COUNTS = 0, 1, 2, 3, 4
AT_PLAN_MODE, AT_PLAN_BYTES, AT_PLAN_LAUNCHES, AT_PLAN_KERNEL, AT_PLAN_SLOTS = 0, 1, 2, 3, 4

# dad_rank_metrics (dad.h DAD_RK_*): the int64 slots of a column's counts, the float64 slots of its values, the flag
# bits, the limits
(RK_MEMBERS, RK_POSITIVES, RK_NONFINITE, RK_RUNS, RK_U2, RK_ACCEPTED, RK_ACCEPTED_POS, RK_VALID_AUROC,
 RK_COUNTS) = range(9)
RK_AUROC, RK_AP, RK_AURC, RK_KEY_MEAN, RK_KEY_STD, RK_KEY_MIN, RK_KEY_MAX, RK_VALUES = 0, 1, 2, 3, 4, 5, 6, 8
RK_MEMBER, RK_POSITIVE = 1, 2
RK_MAX_N, RK_MAX_M, RK_MAX_Q, RK_MAX_BINS, RK_TILE, RK_MAX_CHUNKS, RK_EVAL_COLUMNS = 65536, 16, 8, 64, 256, 8, 10


class DadConfig(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32), ("T", ctypes.c_int32), ("Bn", ctypes.c_int32), ("Tn", ctypes.c_int32),
        ("precision", ctypes.c_int32), ("rng_mode", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("counter", ctypes.c_uint64),
        ("warmup", ctypes.c_int32), ("use_dacp", ctypes.c_int32), ("ecda_on", ctypes.c_int32),
        ("use_entropy", ctypes.c_int32), ("class_aware", ctypes.c_int32), ("dp_world", ctypes.c_int32),
        ("w_kl", ctypes.c_float), ("w_ecda", ctypes.c_float), ("dacp_gamma", ctypes.c_float),
        ("dacp_k", ctypes.c_float), ("dacp_lambda", ctypes.c_float), ("dacp_alpha", ctypes.c_float),
        ("dacp_one_m_alpha", ctypes.c_float), ("fixed_thr", ctypes.c_float),
        ("ecda_att_lambda", ctypes.c_float), ("ecda_gamma", ctypes.c_float), ("ecda_delta", ctypes.c_float),
        ("ls_eps", ctypes.c_float), ("p_drop", ctypes.c_float), ("drop_scale", ctypes.c_float),
        ("feat_p", ctypes.c_float), ("weak_std", ctypes.c_float), ("strong_std", ctypes.c_float),
        ("mask_len", ctypes.c_int32), ("start_hi", ctypes.c_int32), ("clip", ctypes.c_int32),
        ("max_norm", ctypes.c_float), ("lr_step_size", ctypes.c_float), ("bc2_sqrt", ctypes.c_float),
        ("beta1", ctypes.c_float), ("one_m_beta1", ctypes.c_float), ("beta2", ctypes.c_float),
        ("one_m_beta2", ctypes.c_float), ("adam_eps", ctypes.c_float), ("weight_decay", ctypes.c_float),
        ("ema_m", ctypes.c_float), ("ema_one_m", ctypes.c_float),
        ("dacp_beta", ctypes.c_float), ("dacp_one_m_beta", ctypes.c_float),
        ("splits", ctypes.c_int32), ("prepped", ctypes.c_int32), ("ragged", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


def _reserved_word(index, ctype):
    off = DadConfig.reserved.offset + 4 * index
    return property(lambda self: ctype.from_buffer(self, off).value,
                    lambda self, v: setattr(ctype.from_buffer(self, off), "value", v))


# dad.h overlays the three reserved words with the supervised-contrastive term's fields (an anonymous union:
# `reserved` stays addressable, and zeros there still mean a step without the term).  The same overlay here.
DadConfig.SCL_FIELDS = (("scl_on", ctypes.c_int32), ("w_scl", ctypes.c_float), ("scl_tau", ctypes.c_float))
for _i, (_name, _ctype) in enumerate(DadConfig.SCL_FIELDS):
    setattr(DadConfig, _name, _reserved_word(_i, _ctype))


class DadBatch(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("xc", "mc", "yc", "xn", "mn", "nw", "ns", "u", "start", "keep1", "keep2",
                  "rowc", "lenc", "rown", "lenn")]
                + [("xc_dtype", ctypes.c_int32), ("xn_dtype", ctypes.c_int32)])   # STORE_* of the store rows


class DadState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("student", "teacher", "exp_avg", "exp_avg_sq", "grad", "w1bf_student", "w1bf_teacher",
                 "dacp", "tail", "emb", "logits", "losses")]


class DadStepPlanInfo(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in
                 ("splits", "max_splits", "prep_grid", "encode_grid", "ws_nt", "ws_ns", "pool_grid", "tail_grid",
                  "tail_prep", "tail_prep_clean_only", "wgrad_grid", "wgrad_clean", "wgrad_store", "reduce_grid",
                  "prepped", "pending")]
                + [(n, ctypes.c_char_p) for n in ("encode", "tail", "wgrad", "reduce")])


class DadRaggedPlan(ctypes.Structure):
    """dad.h dad_ragged_plan (dad_step_ragged_plan); `ragged_plan()` below fills and unpacks it."""
    _fields_ = ([(n, ctypes.c_int32) for n in
                 ("live_clean", "live_noisy", "enc_grid", "splits", "max_enc_range", "max_split_utts",
                  "enc_capacity", "split_capacity")]
                + [("enc", ctypes.POINTER(ctypes.c_int32)), ("split", ctypes.POINTER(ctypes.c_int32))])


class DadEvalArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("store", "rows", "lens", "labels", "slab_off", "student", "teacher", "emb", "logits", "probs",
                  "score", "pred", "t_emb", "t_logits", "t_pred", "counts", "moments")]
                + [("n", ctypes.c_int64), ("slabs", ctypes.c_int64), ("store_dtype", ctypes.c_int32),
                   ("use_entropy", ctypes.c_int32), ("precision", ctypes.c_int32), ("reserved", ctypes.c_int32)])


class DadWindowArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("store", "rows", "lens", "labels", "slab_off", "params", "win_off", "piece_off", "win_off_host",
                  "w_emb", "w_logits", "w_probs", "w_score", "w_pred", "mean_probs", "mean_pred", "vote_pred",
                  "last_pred", "settle", "switches", "result")]
                + [(n, ctypes.c_int64) for n in ("n", "slabs", "windows", "pieces")]
                + [(n, ctypes.c_int32) for n in ("hop", "span", "mode", "store_dtype", "use_entropy", "precision")])


class DadNoiseArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("store", "rows", "lens", "labels", "slab_off", "params", "noise", "emb", "logits", "probs", "score",
                  "pred", "drift", "kl", "break_level", "counts", "sums")]
                + [("n", ctypes.c_int64), ("slabs", ctypes.c_int64), ("seed", ctypes.c_uint64), ("draw", ctypes.c_uint64),
                   ("sigma", ctypes.c_float * EN_MAX_LEVELS)]
                + [(n, ctypes.c_int32) for n in ("levels", "store_dtype", "use_entropy", "precision")])


class DadModelsArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in ("store", "rows", "lens", "labels", "slab_off")]
                + [("n", ctypes.c_int64), ("slabs", ctypes.c_int64)]
                + [(n, ctypes.c_int32) for n in ("store_dtype", "use_entropy", "precision", "reserved0")]
                + [("models", ctypes.c_void_p * EM_MAX_MODELS), ("weight", ctypes.c_float * EM_MAX_MODELS),
                   ("K", ctypes.c_int32), ("reserved1", ctypes.c_int32)]
                + [(n, ctypes.c_void_p) for n in
                   ("emb", "logits", "probs", "score", "pred", "ens_probs", "ens_score", "ens_pred", "vote_pred",
                    "votes", "n_correct", "counts", "sums")])


class DadInputGradArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("store", "rows", "lens", "slab_off", "params", "dz", "delta_in", "grad", "delta_out", "frame_l1",
                  "counts")]
                + [("n", ctypes.c_int64), ("slabs", ctypes.c_int64), ("alpha", ctypes.c_float), ("radius", ctypes.c_float),
                   ("store_dtype", ctypes.c_int32), ("precision", ctypes.c_int32)])


class DadAttributionArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("store", "rows", "lens", "slab_off", "params", "dz", "baseline", "attr", "frame_attr", "chan_attr",
                  "utt_total", "counts")]
                + [("n", ctypes.c_int64), ("slabs", ctypes.c_int64), ("store_dtype", ctypes.c_int32),
                   ("precision", ctypes.c_int32)])


class DadRankArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in
                 ("key", "flags", "thr", "gammas", "order", "cum_pos", "tie_end", "counts", "values", "quant",
                  "bin_counts", "bin_sum")]
                + [("n", ctypes.c_int64), ("m", ctypes.c_int32), ("Q", ctypes.c_int32), ("B", ctypes.c_int32),
                   ("bin_lo", ctypes.c_float), ("bin_hi", ctypes.c_float), ("reserved", ctypes.c_int32)])


class DadTsneArgs(ctypes.Structure):
    _fields_ = [("max_iter", ctypes.c_int32), ("n_iter_without_progress", ctypes.c_int32),
                ("early_exaggeration", ctypes.c_double), ("learning_rate", ctypes.c_double),
                ("min_grad_norm", ctypes.c_double)]


class DadDomainGapArgs(ctypes.Structure):
    _fields_ = [("class_weights", ctypes.c_float * 4), ("lam", ctypes.c_double), ("gamma", ctypes.c_double),
                ("delta", ctypes.c_double)]      # dad.h dad_domain_gap_args (lam: its `lambda`)


# exported symbols (must match include/dad.h); tests check every one is present
EXPORTS = {
    "dad_abi_version": (ctypes.c_int, []),
    "dad_param_count": (ctypes.c_size_t, []),
    "dad_workspace_bytes": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(ctypes.c_size_t)]),
    "dad_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "dad_encoder_ws_plan": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_encoder_ws_jobs": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                            ctypes.c_int]),
    "dad_step_compute": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                        ctypes.POINTER(DadState), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_step_encode": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                       ctypes.POINTER(DadState), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_step_backward": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                         ctypes.POINTER(DadState), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_step_backward_ahead": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                               ctypes.POINTER(DadState), ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                               ctypes.POINTER(ctypes.c_int)]),
    "dad_step_backward_ahead_split": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                                     ctypes.POINTER(DadState), ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch), ctypes.c_int,
                                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_step_prepare_rows": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch), ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int]),
    "dad_step_plan": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                     ctypes.c_int, ctypes.c_int, ctypes.POINTER(DadStepPlanInfo)]),
    "dad_step_plan_kernels": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch),
                                             ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch), ctypes.c_int,
                                             ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)]),
    "dad_step_ragged_plan": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                            ctypes.POINTER(DadRaggedPlan)]),
    "dad_step_apply": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadState),
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "dad_step": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadBatch), ctypes.POINTER(DadState),
                                ctypes.c_void_p, ctypes.c_void_p]),
    "dad_step_commit": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadState),
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "dad_epoch_end": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.POINTER(DadState), ctypes.c_void_p]),
    "dad_refresh_shadow": (ctypes.c_int, [ctypes.POINTER(DadState), ctypes.c_int, ctypes.c_void_p]),
    "dad_teacher_ema": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_void_p]),
    "dad_encoder_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "dad_encoder_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "dad_encoder_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_collate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_collate_index": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_collate_index_epoch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "dad_predict_head": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "dad_eval_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "dad_eval_split": (ctypes.c_int, [ctypes.POINTER(DadEvalArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_eval_windows_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                           ctypes.c_int64, ctypes.c_int]),
    "dad_eval_windows": (ctypes.c_int, [ctypes.POINTER(DadWindowArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_eval_noise_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "dad_eval_noise": (ctypes.c_int, [ctypes.POINTER(DadNoiseArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_eval_noise_draws": (ctypes.c_int, [ctypes.POINTER(DadNoiseArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_eval_models_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "dad_eval_models": (ctypes.c_int, [ctypes.POINTER(DadModelsArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_input_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "dad_input_grad": (ctypes.c_int, [ctypes.POINTER(DadInputGradArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_attribution_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "dad_attribution": (ctypes.c_int, [ctypes.POINTER(DadAttributionArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_attribution_plan": (ctypes.c_int, [ctypes.POINTER(DadAttributionArgs), ctypes.POINTER(ctypes.c_int64)]),
    "dad_augment": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_certainty_scores": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "dad_dacp_mask": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "dad_ecda_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "dad_ecda_loss": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_rng_draws": (ctypes.c_int, [ctypes.POINTER(DadConfig), ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "dad_trace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dad_trace_append": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "dad_cluster_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dad_cluster_metrics": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_cluster_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_cluster_metrics_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_tsne_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dad_tsne_affinities": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_tsne_gradient": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_tsne_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_tsne_gradient_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "dad_tsne_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(DadTsneArgs),
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_domain_gap_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dad_domain_gap_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_domain_gap": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.POINTER(DadDomainGapArgs), ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "dad_domain_gap_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int64, ctypes.POINTER(DadDomainGapArgs), ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_knn_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dad_knn_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_knn": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_knn_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "dad_knn_vote": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_trustworthiness": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_trustworthiness_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_void_p]),
    "dad_scl_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dad_scl_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_scl": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_scl_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "dad_rank_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dad_rank_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dad_rank_metrics": (ctypes.c_int, [ctypes.POINTER(DadRankArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "dad_rank_metrics_chunked": (ctypes.c_int, [ctypes.POINTER(DadRankArgs), ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "dad_rank_eval_columns": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dad_timing_start": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "dad_timing_kernels": (ctypes.c_int, [ctypes.c_uint]),
    "dad_timing_reset": (ctypes.c_int, []),
    "dad_timing_stop": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "dad_comm_unique_id_bytes": (ctypes.c_int, []),
    "dad_comm_get_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "dad_comm_init": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "dad_comm_allreduce_grad": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(DadState), ctypes.c_void_p]),
    "dad_comm_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "dad_comm_allreduce_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dad_comm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
}

# Entry points added without an ABI bump: a library of the same ABI version built before them loads, and
# the feature that needs one reports the stale build when it is asked for (require()).
OPTIONAL_EXPORTS = ("dad_step_ragged_plan", "dad_step_plan_kernels", "dad_trace_bytes", "dad_trace_append",
                    "dad_cluster_workspace_bytes", "dad_cluster_metrics", "dad_cluster_plan",
                    "dad_cluster_metrics_chunked", "dad_tsne_workspace_bytes", "dad_tsne_affinities",
                    "dad_tsne_gradient", "dad_tsne_plan", "dad_tsne_gradient_chunked", "dad_tsne_run",
                    "dad_domain_gap_workspace_bytes", "dad_domain_gap_plan", "dad_domain_gap",
                    "dad_domain_gap_chunked", "dad_knn_workspace_bytes", "dad_knn_plan", "dad_knn", "dad_knn_chunked",
                    "dad_knn_vote", "dad_trustworthiness", "dad_trustworthiness_chunked",
                    "dad_scl_workspace_bytes", "dad_scl_plan", "dad_scl", "dad_scl_chunked",
                    "dad_eval_windows_workspace_bytes", "dad_eval_windows",
                    "dad_eval_noise_workspace_bytes", "dad_eval_noise", "dad_eval_noise_draws",
                    "dad_input_grad_workspace_bytes", "dad_input_grad",
                    "dad_attribution_workspace_bytes", "dad_attribution", "dad_attribution_plan",
                    "dad_rank_workspace_bytes", "dad_rank_plan", "dad_rank_metrics", "dad_rank_metrics_chunked",
                    "dad_rank_eval_columns", "dad_eval_models_workspace_bytes", "dad_eval_models")

# per-kernel timing slots (dad.h DAD_TK_*)
TK_NAMES = ["encode", "pool", "tail", "wgrad", "reduce", "optim"]

_LIB = None


class DadError(RuntimeError):
    pass


def lib():
    """Load libdad_hip.so (in-tree).  Raises if it is missing: build it with _build.build()."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.lib_path(os.environ.get("DAD_LIB_VARIANT") or None)
    if not os.path.exists(path):
        raise DadError("libdad_hip.so not built (%s); run __graft_entry__.build() or "
                       "python -m <pkg>._build" % path)
    L = ctypes.CDLL(path)
    if not hasattr(L, "dad_abi_version"):
        raise DadError("%s predates ABI 6 (no dad_abi_version): rebuild it (__graft_entry__.build())" % path)
    for name, (res, args) in EXPORTS.items():
        if name in OPTIONAL_EXPORTS and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    ver = L.dad_abi_version()
    if ver != DAD_ABI_VERSION:
        raise DadError("%s was built for ABI %d, this binding needs ABI %d: rebuild it (__graft_entry__.build())"
                       % (path, ver, DAD_ABI_VERSION))
    _LIB = L
    return L


def require(name, what):
    """The optional entry point `name` (OPTIONAL_EXPORTS), or DadError: the library predates `what`."""
    L = lib()
    if not hasattr(L, name):
        raise DadError("%s has no %s, which %s needs: rebuild it (__graft_entry__.build())"
                       % (_build.lib_path(os.environ.get("DAD_LIB_VARIANT") or None), name, what))
    return getattr(L, name)


def ragged_plan(cfg, lenc, lenn, cus):
    """dad_step_ragged_plan for host length lists: {'live_clean', 'live_noisy', 'max_enc_range',
    'max_split_utts', 'enc': [(teacher, first live job, count)], 'split': [(first, end)]}."""
    fn = require("dad_step_ragged_plan", "the ragged plan")
    out = DadRaggedPlan()
    lc = (ctypes.c_int32 * max(len(lenc), 1))(*[int(v) for v in lenc])
    ln = None if lenn is None else (ctypes.c_int32 * max(len(lenn), 1))(*[int(v) for v in lenn])
    rc = fn(cfg, lc, ln, int(cus), out)      # sizes first: no arrays yet (DAD_E_ARG)
    if rc != E_ARG or out.enc_grid <= 0:
        check(rc if rc else E_ARG, "dad_step_ragged_plan")
    enc = (ctypes.c_int32 * (3 * out.enc_grid))()
    split = (ctypes.c_int32 * (2 * max(out.splits, 1)))()
    out.enc, out.split = enc, split
    out.enc_capacity, out.split_capacity = out.enc_grid, max(out.splits, 1)
    check(fn(cfg, lc, ln, int(cus), out), "dad_step_ragged_plan")
    return {"live_clean": out.live_clean, "live_noisy": out.live_noisy, "max_enc_range": out.max_enc_range,
            "max_split_utts": out.max_split_utts,
            "enc": [tuple(enc[3 * i:3 * i + 3]) for i in range(out.enc_grid)],
            "split": [tuple(split[2 * i:2 * i + 2]) for i in range(out.splits)]}


def check(rc, what=""):
    if rc != 0:
        msg = lib().dad_error_string(rc)
        raise DadError("%s failed: %s (%d)" % (what, msg.decode() if msg else "?", rc))


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class KernelTimer:
    """dad_timing_start / dad_timing_stop: mean duration (ms) per kernel of the fused step over
    every `every`-th step while active.  `stop()` returns {name: (mean_ms, n_steps)}."""

    def __init__(self, every=4, max_steps=256, kernels=None):
        """kernels: names (TK_NAMES) to time, default all; each recorded event costs stream time.
        One timer at a time: dad_timing_start refuses (DadError) while another is active."""
        check(lib().dad_timing_start(int(every), int(max_steps)), "dad_timing_start")
        if kernels is not None:
            mask = 0
            for k in kernels:
                mask |= 1 << TK_NAMES.index(k)
            check(lib().dad_timing_kernels(mask), "dad_timing_kernels")
        self.active = True

    def reset(self):
        """dad_timing_reset: the steps so far (a warm-up) are not counted; the events stay created."""
        check(lib().dad_timing_reset(), "dad_timing_reset")

    def stop(self):
        n = len(TK_NAMES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int * n)()
        self.active = False
        check(lib().dad_timing_stop(ms, cnt, n), "dad_timing_stop")
        return {TK_NAMES[k]: (ms[k] / cnt[k], cnt[k]) for k in range(n) if cnt[k] > 0}
