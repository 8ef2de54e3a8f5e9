/*
 * dad.h — C ABI of the MI355X-native DAD (Dynamic Asymmetric Distillation) train step.
 *
 * The reference (TMZZ22331/Robust-Speech-Emotion-Recognition-via-Dynamic-Asymmetric-
 * Distillation-in-Noisy-Environments) is pure Python/PyTorch with no FFI; its operator
 * surface for the hot path is the Python object API listed in SURVEY.md §8(b).  Each
 * entry point below names the reference interface it replaces (I/ = IEMOCAP/DAD-train-
 * IEMOCAP/, identical in CASIA/ and EMODB/ up to the differences resolved by dad_config).
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors in the
 *     Python host layer); sizes are explicit; no allocation, no host synchronisation,
 *     enqueue-only on `stream` (a hipStream_t), graph-capturable;
 *   - return 0 on success, a hipError_t value, or a DAD_E_* code; no exceptions cross;
 *   - reentrant across streams; not thread-safe on one shared state.
 *   - fixed model dims: INPUT_DIM 768, HIDDEN_DIM 256, NUM_CLASSES 4 (I/config.py:54-56).
 */
#ifndef DAD_ABI_H_
#define DAD_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAD_ABI_VERSION 10

/* error codes (besides hipError_t values) */
#define DAD_OK 0
#define DAD_E_ARG 1001        /* null pointer / invalid scalar */
#define DAD_E_SHAPE 1002      /* B/T out of the supported range */
#define DAD_E_COMM 1003       /* RCCL failure */
#define DAD_E_UNSUPPORTED 1004

#define DAD_INPUT_DIM 768
#define DAD_HIDDEN_DIM 256
#define DAD_NUM_CLASSES 4
#define DAD_MAX_BATCH 1024
/* flat parameter vector [W1 (256x768) | b1 (256) | W2 (4x256) | b2 (4)] — the student
 * (or teacher) half of SSRLModel.parameters() (I/model.py:101-122) */
#define DAD_NPARAM (256 * 768 + 256 + 4 * 256 + 4)
/* per-step extras appended to the gradient buffer so ONE all-reduce carries them:
 * [0,4) DACP floored thresholds tau' (mean over ranks), [4,8) per-class certainty
 * sums, [8,12) per-class counts, [12,16) losses (total, ce, kl, ecda) */
#define DAD_GRAD_EXTRA 16
#define DAD_GRAD_FLOATS (DAD_NPARAM + DAD_GRAD_EXTRA)
/* persistent DACPManager state (I/utils.py:384-398): [0,4) tau (ema_thresholds),
 * [4,8) Q (class_quality_scores), [8,12) epoch score sums, [12,16) epoch counts,
 * [16,20) calibrated anchors */
#define DAD_DACP_FLOATS 20
#define DAD_NORM_BLOCKS 1024

/* per-step outputs ("tail" buffer): header then per-sample arrays */
#define DAD_TAIL_HDR 64
#define DAD_T_TOTAL 0
#define DAD_T_CE 1
#define DAD_T_KL 2
#define DAD_T_ECDA 3
#define DAD_T_SCL 4           /* dad_config.scl_on: the supervised-contrastive loss of this rank's batch; else 0, as
                                 the reference hard-wires it (C/train_CASIA.py:442, E/train_emodb.py:404) */
#define DAD_T_MSUM 5
#define DAD_T_CLIPNORM 6
#define DAD_T_CLIPCOEF 7
#define DAD_T_W 8             /* [4] DACP class weights W_c */
#define DAD_T_TAU_BEFORE 12   /* [4] */
#define DAD_T_TAU_AFTER 16    /* [4] */
#define DAD_T_FLOORED 20      /* [4] */
#define DAD_T_ECDA_TERM 24    /* [4] att_c * (mmd_c + gamma comp_c + delta rep) */
#define DAD_T_ECDA_GATE 28    /* [4] */
#define DAD_T_KL_ON 32
#define DAD_T_ECDA_ON 33
#define DAD_T_RANGE 34        /* u32 bits, sticky (only the caller clears them; the buffer starts zero-filled):
                                 DAD_RANGE_NONFINITE: a step's pooled embedding or logit, or the step's gradient,
                                 was not finite (FP16: an encoder operand beyond +-65504; any mode: non-finite
                                 features; the gradient: its global norm, as dad_step_apply takes it, is NaN, inf
                                 or beyond FLT_MAX -- that step's update was skipped);
                                 DAD_RANGE_POOL_TIMEOUT: a tail / class block gave up waiting for the tail
                                 launch's fused pooling (~0.2 s); that step's update was skipped (its total loss
                                 is NaN).  dad_step_apply skips the update of any step whose total loss or
                                 gradient norm is not finite. */
#define DAD_RANGE_NONFINITE 1u
#define DAD_RANGE_POOL_TIMEOUT 2u
#define DAD_T_TAU_HAT 40      /* [4] batch quantile thresholds */
/* after the header (noisy batch, Bn rows): score[Bn], pred[Bn] (as float), mask[Bn], q[Bn][4] */
#define DAD_TAIL_FLOATS(Bn) (DAD_TAIL_HDR + (Bn) * (3 + DAD_NUM_CLASSES))

/* FP32: exact-f32 MFMA (the reference's arithmetic, parity mode).  FP16 / BF16: the encoder and
 * weight-gradient GEMMs on 16-bit operands (fp16: 11-bit significand, the throughput mode that
 * meets the 1e-4 loss/logit bound; bf16: 8-bit) with fp32 accumulation; everything else fp32. */
enum dad_precision { DAD_PREC_FP32 = 0, DAD_PREC_BF16 = 1, DAD_PREC_FP16 = 2 };
enum dad_rng_mode { DAD_RNG_EXPLICIT = 0, DAD_RNG_COUNTER = 1 };

/* Every scalar the step reads from the reference's config module, resolved by the host
 * at CALL time (the reference re-reads config inside the functions, I/utils.py:410,567,
 * and the ablation runners mutate it between runs, I/run_granular_ablations.py:25-30).
 * Float scalars are the float32 values torch would use for the python-float operands. */
typedef struct dad_config {
  int32_t B, T;                 /* clean batch: utterances, padded frames (batch max length) */
  int32_t Bn, Tn;               /* noisy batch (collated independently, I/train.py:479-483) */
  int32_t precision;            /* dad_precision */
  int32_t rng_mode;             /* dad_rng_mode */
  uint64_t seed, counter;       /* counter-RNG key material (counter = global step) */
  int32_t warmup;               /* epoch < WARMUP_EPOCHS: CE only, no EMA (I/train.py:402,491) */
  int32_t use_dacp;             /* DACP vs fixed threshold (I/train.py:414-420) */
  int32_t ecda_on;              /* USE_ECDA && weight_ecda > 0 (I/train.py:450) */
  int32_t use_entropy;          /* USE_ENTROPY_IN_SCORE (I/utils.py:415) */
  int32_t class_aware;          /* USE_CLASS_AWARE_MMD (I/utils.py:579) */
  int32_t dp_world;             /* ranks whose grads are all-reduced (1 = single GPU) */
  float w_kl, w_ecda;           /* update_loss_weights (I/train.py:380-395) */
  float dacp_gamma;             /* quantile level gamma_e (I/utils.py:471-473) */
  float dacp_k, dacp_lambda, dacp_alpha, dacp_one_m_alpha;
  float fixed_thr;              /* FIXED_CONFIDENCE_THRESHOLD */
  float ecda_att_lambda, ecda_gamma, ecda_delta;
  float ls_eps;                 /* label smoothing (I/train.py:364) */
  float p_drop, drop_scale;     /* classifier dropout p, float32(1)/float32(1-p) */
  float feat_p;                 /* strong-aug feature dropout rate (I/utils.py:325,343) */
  float weak_std, strong_std;
  int32_t mask_len, start_hi;   /* int(Tn*ratio), max(1, Tn-mask_len+1) (I/utils.py:365,370) */
  int32_t clip;                 /* GRADIENT_CLIPPING */
  float max_norm;
  float lr_step_size;           /* lr / (1 - beta1^t)      (torch Adam single-tensor) */
  float bc2_sqrt;               /* sqrt(1 - beta2^t) */
  float beta1, one_m_beta1, beta2, one_m_beta2, adam_eps, weight_decay;
  float ema_m, ema_one_m;       /* EMA_MOMENTUM, 1-EMA_MOMENTUM (I/model.py:219) */
  float dacp_beta, dacp_one_m_beta;   /* epoch-end quality smoothing (I/utils.py:433-436) */
  int32_t splits;               /* weight-gradient split-K factor (0 = auto) */
  int32_t prepped;              /* FP16/BF16: 1 = the previous step's dad_step_backward_ahead prepared this
                                   batch's 16-bit rows (it reported *prepped = 1 for this cfg and batch), so
                                   the encoder skips the preparation; 0 = prepare them in this step */
  int32_t ragged;               /* FP16/BF16 store-mode steps: 1 = ragged mode, no launch of the step reads, computes or
                                   writes anything for a 32-frame slab that lies wholly past its utterance's end
                                   (slab c of utterance b is live iff c < ceil(len_b / 32), len_b = dad_batch.lenc /
                                   lenn[b], read on the device; len_b = 0: no live slab).  Both batches must be store
                                   batches (DAD_E_ARG otherwise; DAD_PREC_FP32: DAD_E_UNSUPPORTED), and mc / mn must
                                   mark every frame t >= len_b as padding, as dad_collate_index writes them (frames
                                   inside len_b may be marked too).  Buffer layouts, dense slab indices, RNG streams
                                   and outputs are those of the dense step: the forward pass is bit-identical, the
                                   gradient differs only by the order in which split partials are summed (not at all
                                   when every slab is live).  A set prepared ragged is read by a ragged step only
                                   (preparation ahead needs next_cfg->ragged == cfg->ragged).  0 = dense (the field
                                   was reserved[0], always 0, before) */
  /* The supervised-contrastive term (dad_scl below) in the step.  The three words were reserved[3], always 0, and
   * stay addressable under that name: zeros mean what they meant, a step without the term.
   *   scl_on   1: a post-warm-up step enqueues dad_scl's launches behind its tail launch, on the pre-dropout student
   *            embeddings of the B clean rows (class yc) and of the Bn strong rows whose DACP mask is set (class =
   *            the teacher's pseudo-label); it writes tail[DAD_T_SCL], adds w_scl dL/de to the step's dL/de and
   *            w_scl L to the total loss.  The workspace grows by dad_scl's (dad_workspace_bytes counts it).
   *            Each DP rank contrasts within its own batch; tail[DAD_T_SCL] is the local rank's value.
   *   w_scl    TARGET_SCL_WEIGHT once the epoch reaches SCL_START_EPOCH
   *   scl_tau  the temperature, > 0 and finite when scl_on (DAD_E_ARG otherwise) */
  union {
    int32_t reserved[3];
    struct {
      int32_t scl_on;
      float w_scl;
      float scl_tau;
    };
  };
} dad_config;

/* One clean + one noisy collated batch (I/dataload_noisy.py:124-129 format). */
typedef struct dad_batch {
  const void* xc;               /* [B][T][768] clean features (f32; store mode: rows of xc_dtype) */
  const uint8_t* mc;            /* [B][T] padding mask, 1 = pad */
  const int64_t* yc;            /* [B] clean labels */
  const void* xn;               /* [Bn][Tn][768] noisy features (f32; store mode: rows of xn_dtype) */
  const uint8_t* mn;            /* [Bn][Tn] */
  /* DAD_RNG_EXPLICIT only (parity mode; NULL otherwise): the reference's six draws */
  const float* nw;              /* [Bn][Tn][768] randn for weak aug */
  const float* ns;              /* [Bn][Tn][768] randn for strong aug */
  const float* u;               /* [768] rand for feature dropout */
  const int64_t* start;         /* [Bn] temporal-mask starts */
  const uint8_t* keep1;         /* [B][256] classifier dropout keep mask, clean pass */
  const uint8_t* keep2;         /* [Bn][256] classifier dropout keep mask, strong pass */
  /* STORE MODE, per batch (rowc+lenc for the clean one, rown+lenn for the noisy one; NULL =
   * padded): xc / xn point at a feature store [frames][768] (FeatureStore, the device-
   * resident data path) instead of a padded [B][T][768] batch, and
   * frame t < T of utterance b is store row rowc[b] + min(t, lenc[b] - 1) (rown/lenn for the
   * noisy batch).  The encoder's LDS-DMA reads the rows in place: collation never copies the
   * features.  mc / mn / yc keep their [B][T] / [B] meaning (dad_collate_index builds them
   * together with rowc / lenc). */
  const int64_t* rowc;          /* [B] store row of frame 0 of each clean utterance */
  const int32_t* lenc;          /* [B] its frame count (rows >= it are padding) */
  const int64_t* rown;          /* [Bn] */
  const int32_t* lenn;          /* [Bn] */
  /* ABI 10: the element type of the store rows, DAD_STORE_F32 (0) / DAD_STORE_F16 / DAD_STORE_BF16, of the
   * clean store (with rowc) and the noisy store (with rown); the two stores may differ.  FP16 / BF16 steps
   * read 16-bit rows in place wherever they prepare rows (dad_step, dad_step_encode, dad_step_compute,
   * dad_step_backward_ahead[_split] for the next batch, dad_step_prepare_rows): each value is widened
   * exactly to f32 and then treated as an f32 store row (rows of the operands' own type are copied as
   * bytes), so a 16-bit store gives the results of its widened f32 copy.  FP32 steps: DAD_E_UNSUPPORTED.
   * A padded batch (rowc / rown NULL) is f32: a non-zero value there is DAD_E_ARG. */
  int32_t xc_dtype, xn_dtype;
} dad_batch;

/* Persistent training state, all caller-owned device buffers. */
typedef struct dad_state {
  float* student;               /* [DAD_NPARAM] */
  float* teacher;               /* [DAD_NPARAM] */
  float* exp_avg;               /* [DAD_NPARAM] Adam m */
  float* exp_avg_sq;            /* [DAD_NPARAM] Adam v */
  float* grad;                  /* [DAD_GRAD_FLOATS] grads (+extras); the DP all-reduce buffer */
  uint16_t* w1bf_student;       /* [256*768] 16-bit shadow of student W1 (fp16 in FP16 steps, else bf16) */
  uint16_t* w1bf_teacher;       /* [256*768] 16-bit shadow of teacher W1 */
  float* dacp;                  /* [DAD_DACP_FLOATS] */
  float* tail;                  /* [DAD_TAIL_FLOATS(Bn)] per-step outputs */
  float* emb;                   /* [B+2*Bn][256] e_clean [B], e_teacher [Bn], e_strong [Bn] */
  float* logits;                /* [B+2*Bn][4]   z_clean, z_teacher, z_strong */
  float* losses;                /* [4] (optional) total, ce, kl, ecda of this step (rank mean) */
} dad_state;

/* --- sizing ------------------------------------------------------------------------ */
/* DAD_ABI_VERSION the library was built with (ABI 10; 9 lacked dad_batch.xc_dtype / xn_dtype, 8 dad_step_plan, 7 dad_eval_split, 6 dad_timing_reset): a binding compares it with the header's
 * value when it loads the library, so a stale build fails at load instead of at a call. */
int dad_abi_version(void);
size_t dad_param_count(void);
/* Step workspace bytes for cfg's geometry and precision, plus dad_scl's workspace for B + Bn rows behind them when
 * cfg->scl_on (no initialisation needed). */
int dad_workspace_bytes(const dad_config* cfg, size_t* bytes);
const char* dad_error_string(int code);
/* Host-only planning of the 16-bit (FP16/BF16) encoder grid (no device call): teacher / student workgroups
 * for a device of `cus` compute units and the most 32-row jobs any workgroup's range holds
 * (always <= 256, the kernel's per-workgroup table).  Diagnostics and tests. */
int dad_encoder_ws_plan(const dad_config* cfg, int cus, int* nt, int* ns, int* max_jobs);
/* Host-only: the 16-bit encoder's job assignment for a device of `cus` CUs: for every workgroup
 * wg of the grid, jobs[4wg..4wg+3] = (teacher 1/0, first job, job stride, job count); student jobs
 * j < B*ceil(T/32) are clean slabs, the rest strong slabs.  `capacity` = ints available at jobs.
 * The grid is nt + ns of dad_encoder_ws_plan: usually `cus`, more when a range would exceed the
 * kernel's 256-job table (very long batches), so size jobs as 4 * (nt + ns).  Returns the grid
 * size (> 0), DAD_E_ARG when 4 * grid > capacity (nothing written), or another DAD_E_* code.
 * Diagnostics and tests.  (ABI 5: `capacity` added.) */
int dad_encoder_ws_jobs(const dad_config* cfg, int cus, int* jobs, int capacity);

/* --- fused train step ---------------------------------------------------------------
 * Replaces the body of Trainer.train_epoch's loop (I/train.py:484-492):
 *   train_step (I/train.py:397-471) + backward + clip_grad_norm_ + Adam.step + update_teacher_ema.
 * dad_step_compute: encoder passes, losses, DACP mask, analytic backward -> state->grad.
 * dad_step_apply:   global-norm clip, Adam (L2 decay), teacher EMA, DACP state commit,
 *                   16-bit W1 shadow refresh.  A DP caller all-reduces state->grad in between.
 * dad_step = compute + apply (single GPU). */
int dad_step_compute(const dad_config* cfg, const dad_batch* batch, const dad_state* st,
                     void* workspace, void* stream);
/* dad_step_compute = dad_step_encode (the fused augmentation + three encoder GEMMs +
 * pooling partials, one launch) followed by dad_step_backward (pool, losses, DACP,
 * ECDA, analytic backward, weight gradient, reduction); split so callers can time the
 * encoder launch on their stream. */
int dad_step_encode(const dad_config* cfg, const dad_batch* batch, const dad_state* st,
                    void* workspace, void* stream);
int dad_step_backward(const dad_config* cfg, const dad_batch* batch, const dad_state* st,
                      void* workspace, void* stream);
/* dad_step_backward + the NEXT step's row preparation (FP16/BF16: the augmentation and 16-bit
 * conversion of next_batch under next_cfg, weight-independent) on the CUs this step's tail launch
 * leaves idle.  *prepped = 1 when it was enqueued: the next step then passes cfg->prepped = 1 with
 * the same next_cfg scalars and next_batch pointers, whose contents must not change in between.
 * *prepped = 0 (and nothing extra enqueued) unless: 16-bit precision, the tail runs as the
 * wave-centric launch (B, Bn <= 64, class-aware MMD), next_cfg has this cfg's geometry and
 * precision and the other counter parity.  Replaces nothing in the reference: its loop draws the
 * augmentation inside train_step (I/train.py:406-410,439); the draws are the same streams. */
int dad_step_backward_ahead(const dad_config* cfg, const dad_batch* batch, const dad_state* st,
                            void* workspace, void* stream, const dad_config* next_cfg,
                            const dad_batch* next_batch, int* prepped);
/* dad_step_backward_ahead with parts of the next batch's rows left to the caller, for the data-parallel
 * step (ABI 6): `defer` (DAD_PREP_CLEAN and/or DAD_PREP_NOISY) names the parts this step's launches skip
 * (deferred clean rows: the weight gradient runs as the plain GEMM; deferred noisy rows: the tail launch
 * ends with its tail and class blocks); *pending = the parts the caller must prepare with
 * dad_step_prepare_rows(next_cfg, next_batch, workspace, any stream, *pending) before the next step's
 * dad_step_encode (order the streams with events).  A DP caller issues it on a second stream under the
 * gradient all-reduce, where the CUs would idle.  *prepped as for dad_step_backward_ahead (*pending = 0
 * when *prepped = 0). */
#define DAD_PREP_CLEAN 1
#define DAD_PREP_NOISY 2
int dad_step_backward_ahead_split(const dad_config* cfg, const dad_batch* batch, const dad_state* st,
                                  void* workspace, void* stream, const dad_config* next_cfg,
                                  const dad_batch* next_batch, int defer, int* prepped, int* pending);
/* FP16/BF16: the augmentation and 16-bit conversion of (cfg, batch)'s rows (parts: DAD_PREP_CLEAN and/or
 * DAD_PREP_NOISY) into the workspace's prepared set of cfg->counter's parity -- the set the step with this
 * cfg reads (dad_prep; the draws of cfg's counter).  DAD_E_UNSUPPORTED in FP32. */
int dad_step_prepare_rows(const dad_config* cfg, const dad_batch* batch, void* workspace, void* stream, int parts);
/* Host-only (ABI 9): the launches the step with cfg makes on a device of `cus` compute units -- the plan
 * the step itself enqueues from -- when its backward is dad_step_backward_ahead_split(.., next_cfg,
 * next_batch, defer, ..) (next_cfg = next_batch = NULL, defer = 0: dad_step_backward).  No device call;
 * the batch pointers are only tested for NULL, never followed.  A grid of 0 = that launch is not made;
 * kernel names are static strings and name families: the plan resolves every launch to its exact entry point
 * (dad_step_plan_kernels below), and this struct reports the kernel that entry point stands in for -- itself,
 * or for an `_s16` sibling (the same kernel with the row loads in an fp16 / bf16 store's type, ABI 10) and
 * an `_rg` sibling (a ragged step's kernel) the f32 / dense kernel of the same grid.  This query has no
 * current batch: it plans for a padded f32 one.  Returns cfg's validation code, or DAD_E_ARG for cus < 2, out = NULL
 * or defer bits outside DAD_PREP_*; a next step that does not qualify for preparation ahead is no
 * error (prepped = 0).  Diagnostics and tests. */
typedef struct dad_step_plan_info {
  int32_t splits, max_splits;   /* weight-gradient split-K factor of this step; the one the workspace is sized for */
  int32_t prep_grid;            /* standalone dad_prep of this step's rows before the encoder (cfg->prepped = 0) */
  int32_t encode_grid;
  int32_t ws_nt, ws_ns;         /* 16-bit encoder: teacher / student workgroups (dad_encoder_ws_plan) */
  int32_t pool_grid;            /* separate dad_pool; 0: the tail launch pools */
  int32_t tail_grid;
  int32_t tail_prep;            /* DAD_PREP_* parts of the next batch's rows the tail launch prepares */
  int32_t tail_prep_clean_only; /* that set holds clean rows only */
  int32_t wgrad_grid;
  int32_t wgrad_clean;          /* the weight gradient converts the next batch's clean rows */
  int32_t wgrad_store;          /* ... gathered through that batch's rowc / lenc table */
  int32_t reduce_grid;
  int32_t prepped, pending;     /* as dad_step_backward_ahead_split reports them */
  const char* encode;           /* dad_encode_wp_f16 / dad_encode_wp / dad_encode_f32 */
  const char* tail;             /* dad_tail_ecda_w / dad_tail_ecda / dad_tail */
  const char* wgrad;            /* dad_wgrad_direct[_f16][_cp|_cps] / dad_wgrad_f32 */
  const char* reduce;           /* dad_reduce_w / dad_reduce */
} dad_step_plan_info;
int dad_step_plan(const dad_config* cfg, const dad_config* next_cfg, const dad_batch* next_batch, int defer,
                  int cus, dad_step_plan_info* out);
/* Host-only (ABI 10, added without a bump): the exact entry points of the same plan, the `_s16` / `_rg`
 * siblings named as such, in launch order; out[i] = NULL where that launch is not made.  `batch` is this
 * step's (its row types choose the standalone preparation; only the struct's own fields are read), or NULL
 * for a padded f32 batch.  Static strings, no device call.  Returns dad_step_plan's codes, and
 * for a batch whose row types the step refuses the step's code (DAD_E_ARG / DAD_E_UNSUPPORTED).
 * Diagnostics and tests. */
#define DAD_STEP_LAUNCHES 6   /* prep, encode, pool, tail, wgrad, reduce: launch order */
int dad_step_plan_kernels(const dad_config* cfg, const dad_batch* batch, const dad_config* next_cfg,
                          const dad_batch* next_batch, int defer, int cus, const char* out[DAD_STEP_LAUNCHES]);
/* Host-only: how a ragged step (cfg->ragged = 1, see dad_config) on a device of `cus` compute units divides
 * its live slabs, computed from HOST copies of the two length arrays (lenc [B], lenn [Bn]; lenn may be NULL
 * in a warm-up step) by the functions the kernels call on the device lengths.  Live lists: teachers run the
 * live weak slabs, students the live clean slabs and then the live strong slabs, both in (utterance, slab)
 * order; the weight gradient runs the student list.
 *   enc[3 wg ..]   (teacher 1/0, first live job, count) of encoder workgroup wg < enc_grid (= ws_nt + ws_ns of
 *                  dad_step_plan: the grid does not depend on the lengths); live job k of a teacher is entry k
 *                  of the live weak list, of a student entry k of the student list
 *   split[2 s ..]  [first, end) of weight-gradient split s < splits in the student list
 * enc_capacity / split_capacity (in): the triples / pairs the caller's arrays hold.  enc_grid and splits are
 * written first; DAD_E_ARG (nothing else written) when a capacity is too small.  The encoder's shares are even
 * by live 16-row sub-slabs, as the dense step's, unless one would exceed the kernel's 256-job table (many
 * utterances of at most 16 frames sorted together): that role's jobs are then split evenly by count.  So
 * max_enc_range never exceeds 256, and max_split_utts never 64, the weight gradient's per-split table.  No
 * device call.
 * Diagnostics and tests. */
typedef struct dad_ragged_plan {
  int32_t live_clean, live_noisy;       /* live slabs per branch (weak = strong = live_noisy) */
  int32_t enc_grid, splits;
  int32_t max_enc_range;                /* the most live jobs any encoder workgroup runs */
  int32_t max_split_utts;               /* the most utterances any weight-gradient split touches */
  int32_t enc_capacity, split_capacity; /* in */
  int32_t* enc;                         /* in: [3 * enc_capacity] */
  int32_t* split;                       /* in: [2 * split_capacity] */
} dad_ragged_plan;
int dad_step_ragged_plan(const dad_config* cfg, const int32_t* lenc, const int32_t* lenn, int cus,
                         dad_ragged_plan* out);
int dad_step_apply(const dad_config* cfg, const dad_state* st, void* workspace, void* stream);
int dad_step(const dad_config* cfg, const dad_batch* batch, const dad_state* st,
             void* workspace, void* stream);
/* Trainer.train_step alone (I/train.py:397-471) for callers that keep their own
 * backward/clip/optimizer/EMA (I/train.py:486-492): after dad_step_compute, commits the
 * DACP state update of calculate_mask (I/utils.py:485-505) and writes st->losses; the
 * pre-clip gradient of total_loss stays in st->grad (rank mean when dp_world > 1). */
int dad_step_commit(const dad_config* cfg, const dad_state* st, void* workspace, void* stream);

/* DACPManager.update_class_quality_scores_epoch (I/utils.py:430-447) */
int dad_epoch_end(const dad_config* cfg, const dad_state* st, void* stream);
/* --- the confirmation-bias log, appended on the device (csrc/trace.hip) ----------------
 * Replaces the logging loop of Trainer.train_step (I/train.py:425-437): for every row of the noisy batch whose
 * sample id is tracked (Trainer.tracked_sample_indices, I/train.py:279-284) the reference appends
 * {epoch, sample_id, pseudo_label, certainty_score, is_masked_in} to bias_analysis_log, reading the ids with
 * .cpu() and three values per row with .item().  dad_trace_append appends the same entries, in the same order,
 * to a device buffer, from what the step's tail launch left in its tail buffer; the host reads the buffer once,
 * at the end of the run (I/train.py:691-700 writes it out).
 *
 * Trace buffer: int32 words, 16-byte aligned, zero-filled once by the caller; after that only dad_trace_append
 * writes it.  Header, then `capacity` records.
 *
 * Added without an ABI bump (no existing structure or entry point changes): a library of ABI 10 built before
 * them lacks the two symbols, and a binding reports that when a trace is asked for. */
#define DAD_TRACE_HDR_WORDS 4      /* int32: [0] = records OFFERED so far (may exceed capacity; saturates at
                                      2^31 - 1); [1..3] reserved, 0 */
#define DAD_TRACE_REC_WORDS 4      /* int32 epoch | int32 sample_id | int32 label + flags | float certainty score */
#define DAD_TRACE_MASKED_IN 0x100  /* flag in word 2: mask[i] != 0; the pseudo-label is word2 & 0xff */
/* (DAD_TRACE_HDR_WORDS + capacity * DAD_TRACE_REC_WORDS) * 4; host only */
size_t dad_trace_bytes(int64_t capacity);
/* One step's entries.  tail: the step's tail buffer (dad_state.tail, DAD_TAIL_FLOATS(Bn)) after its tail launch
 * was enqueued on `stream`: score = tail[DAD_TAIL_HDR + i], pred = tail[DAD_TAIL_HDR + Bn + i] (as float), mask =
 * tail[DAD_TAIL_HDR + 2 Bn + i].  ids [Bn]: the noisy batch's sample ids (noisy_batch['id']).  tracked: a bitmap
 * of ceil(n_samples / 32) words, bit (id & 31) of word (id >> 5) set = sample id is tracked.  Rows with
 * 0 <= ids[i] < n_samples and their bit set are appended in batch order (ascending i) behind the records already
 * there; rows with an id outside the range are ignored, and such an id never indexes the bitmap.  trace[0]
 * counts every record offered; a record at a position >= capacity is dropped and nothing at or past word
 * DAD_TRACE_HDR_WORDS + capacity * DAD_TRACE_REC_WORDS is written, so the host sees trace[0] > capacity and
 * knows how many were lost.
 * Enqueue-only like every entry point (no host read, no allocation, no synchronisation).  Two appends to one
 * trace MUST be ordered on one stream (or by events): the cursor is read at the kernel's entry and written once
 * at its exit, without atomics.
 * DAD_E_ARG: a NULL pointer, or trace not 16-byte aligned; DAD_E_SHAPE: Bn outside [1, DAD_MAX_BATCH], n_samples
 * outside [1, 2^31 - 1], capacity outside [0, 2^31 - 1]; all checked before anything is launched. */
int dad_trace_append(const float* tail, int Bn, const int64_t* ids, const uint32_t* tracked, int64_t n_samples,
                     int epoch, int32_t* trace, int64_t capacity, void* stream);

/* refresh the 16-bit shadows of W1 after the caller changed student/teacher params
 * (e.g. load_complete_pretrained_weights, I/model.py:143-198): fp16 for precision
 * DAD_PREC_FP16, bf16 otherwise (the format the next step of that precision reads) */
int dad_refresh_shadow(const dad_state* st, int precision, void* stream);

/* SSRLModel.update_teacher_ema (I/model.py:211-223) over flat [W1|b1|W2|b2] vectors:
 * teacher = teacher*ema_m + student*ema_one_m (n floats) */
int dad_teacher_ema(const float* student, float* teacher, size_t n, float ema_m, float ema_one_m, void* stream);

/* --- modular operators (the SSRLModel / utils.py surface) --------------------------
 * Emotion2VecEncoder.forward (I/model.py:18-41): e[B][256] = masked mean of ReLU(x W1^T + b1).
 * workspace: dad_encoder_workspace_bytes(B, T). */
size_t dad_encoder_workspace_bytes(int B, int T);
int dad_encoder_forward(const float* x, const uint8_t* pad, int B, int T, const float* w1,
                        const float* b1, float* e_out, int precision, void* workspace, void* stream);
/* backward of the above w.r.t. W1, b1 given de[B][256] (autograd of I/model.py:28-36);
 * recomputes the ReLU pattern; dw1 [256][768], db1 [256] are overwritten. */
int dad_encoder_backward(const float* x, const uint8_t* pad, int B, int T, const float* w1,
                         const float* b1, const float* de, float* dw1, float* db1,
                         void* workspace, void* stream);

/* --- device-resident data path ---------------------------
 * One padded batch gathered from a feature store resident in HBM.  Replaces the DataLoader's
 * per-sample row slice + .float() (NoisyEmotionDatasetFromArrays.__getitem__,
 * I/dataload_noisy.py:104-115; CleanEmotionDatasetFromArrays.__getitem__, I/dataload_clean.py:
 * 170-176) and its collator (I/dataload_noisy.py:116-129, I/dataload_clean.py:177-193,
 * C/dataload_casia_noisy.py:68-99):
 *   store     [frames][768] features of the whole split, dtype DAD_STORE_*
 *   offsets   [n_samples] int64 first frame of each sample; sizes [n_samples] int32 frames
 *   index     [B] int64 sample indices of this batch (the sampler's order)
 *   T         padded length, >= max(sizes[index]) (the collator's target_size)
 *   feats     [B][T][768] f32 out: sample rows, zeros past each size
 *   pad       [B][T] u8 out: 1 = padding (padding_mask[i, size:] = True)
 *   labels_in [n_samples] int64, labels_out [B] int64: both null for an unlabeled loader
 * An index outside [0, n_samples) yields an all-padding row and label -1 (no read). */
#define DAD_STORE_F32 0
#define DAD_STORE_F16 1
#define DAD_STORE_BF16 2
int dad_collate(const void* store, int store_dtype, const int64_t* offsets, const int32_t* sizes,
                int64_t n_samples, const int64_t* index, int B, int T, float* feats, uint8_t* pad,
                const int64_t* labels_in, int64_t* labels_out, void* stream);

/* Store-mode batch index (see dad_batch): for each b, row_out[b] = offsets[index[b]],
 * len_out[b] = sizes[index[b]] (0 and row 0 for an index outside [0, n_samples)),
 * pad [B][T] and labels exactly as dad_collate writes them -- the collator's outputs without
 * the feature copy. */
int dad_collate_index(const int64_t* offsets, const int32_t* sizes, int64_t n_samples, const int64_t* index,
                      int B, int T, int64_t* row_out, int32_t* len_out, uint8_t* pad,
                      const int64_t* labels_in, int64_t* labels_out, void* stream);
/* dad_collate_index for every batch of an epoch in one launch (the store-mode loader's epoch start):
 * n samples in batch order, sample i of a batch padded to T_i = pad_T[i] (its batch's T) with its
 * pad row at pad + pad_off[i] (T_i bytes); row_out / len_out / labels_out [n].  Per sample the same
 * values dad_collate_index writes. */
int dad_collate_index_epoch(const int64_t* offsets, const int32_t* sizes, int64_t n_samples, const int64_t* index,
                            int64_t n, const int64_t* pad_off, const int64_t* pad_T, int64_t* row_out,
                            int32_t* len_out, uint8_t* pad, const int64_t* labels_in, int64_t* labels_out,
                            void* stream);

/* --- eval path ------------------------------------------------
 * SSRLModel.predict's classifier in eval mode (I/model.py:225-245) on embeddings e [B][256]
 * from dad_encoder_forward, with what validation (I/train.py:522-564) and anchor calibration
 * (I/train.py:317-357) read from it: logits [B][4], softmax probs [B][4], the DACP certainty
 * score [B] (DACPManager.calculate_certainty_scores, I/utils.py:401-430; use_entropy selects
 * max_prob * (1 - H/log2 C) or max_prob) and the argmax pred [B].  Outputs may be NULL. */
int dad_predict_head(const float* e, int B, const float* w2, const float* b2, int use_entropy,
                     float* logits, float* probs, float* score, int64_t* pred, void* stream);

/* --- whole-split evaluation, store-fed (csrc/eval_split.hip; ABI 8) ---------------------
 * Trainer.validate (I/train.py:522-564), the teacher pass of its disagreement rate,
 * Trainer._run_anchor_calibration's statistics (I/train.py:317-357) and the split-wide
 * SSRLModel.get_embeddings (I/model.py:247-265) over EVERY utterance of a feature-store split in
 * one call: the eval-mode forward reads the store rows in place (no padded batch, no mask) and
 * the confusion matrices, the teacher disagreement count and the per-class certainty moments are
 * built on the device.  The caller copies one small result block back.
 *
 * Result block: counts[DAD_EV_COUNTS] int64 and moments[4][DAD_EV_MOMENTS] double. */
#define DAD_EV_CONF_STUDENT 0   /* [4][4] row = label, column = student prediction (labelled utterances) */
#define DAD_EV_CONF_TEACHER 16  /* [4][4] the same for the teacher (zeros without one) */
#define DAD_EV_DISAGREE 32      /* student pred != teacher pred, over all n utterances (0 without a teacher) */
#define DAD_EV_N 33             /* n */
#define DAD_EV_N_LABELLED 34    /* utterances with a label in [0, 4) */
#define DAD_EV_N_SKIPPED 35     /* label outside [0, 4), or labels == NULL (then n) */
#define DAD_EV_N_NONFINITE 36   /* utterances with a student or teacher logit that is not finite (FP16: an
                                   operand beyond +-65504; any mode: non-finite features) */
#define DAD_EV_COUNTS 40        /* int64 slots of the counts block (37..39 reserved, written 0) */
/* moments[c][.] of the student's certainty score over the utterances of true class c, in float64
 * over the float32 scores, two passes in a fixed order (np.mean / np.std ** 2 of the reference's
 * .item() lists); count 0 gives mean = variance = 0 */
#define DAD_EV_MOMENTS 3
#define DAD_EV_M_COUNT 0
#define DAD_EV_M_MEAN 1
#define DAD_EV_M_VAR 2          /* population variance */
/* Utterance i < n is frames [rows[i], rows[i] + lens[i]) of the store (rows need be neither sorted
 * nor unique; lens[i] = 0 reads nothing and gives a zero embedding, logits = b2).  The slab jobs are
 * described by the device prefix slab_off[n + 1] (int32): slab_off[0] = 0, slab_off[i + 1] =
 * slab_off[i] + ceil(lens[i] / 32); `slabs` is its last entry, on the host.  An utterance whose
 * prefix entries disagree with its length gets a zero embedding (nothing is read for it).
 * Per-utterance outputs are optional (NULL = not written).  Two calls on the same inputs write
 * bit-identical outputs (no floating-point atomics). */
typedef struct dad_eval_args {
  const void* store;            /* [frames][768], dtype store_dtype */
  const int64_t* rows;          /* [n] store row of frame 0 */
  const int32_t* lens;          /* [n] frames */
  const int64_t* labels;        /* [n] or NULL */
  const int32_t* slab_off;      /* [n + 1] exclusive prefix of ceil(lens / 32) */
  const float* student;         /* [DAD_NPARAM] flat [W1|b1|W2|b2] */
  const float* teacher;         /* [DAD_NPARAM] or NULL: no teacher pass */
  float* emb;                   /* [n][256] student embeddings */
  float* logits;                /* [n][4] */
  float* probs;                 /* [n][4] */
  float* score;                 /* [n] certainty score (dad_predict_head's) */
  int64_t* pred;                /* [n] first-maximum argmax */
  float* t_emb;                 /* [n][256] teacher */
  float* t_logits;              /* [n][4] */
  int64_t* t_pred;              /* [n] */
  int64_t* counts;              /* [DAD_EV_COUNTS] */
  double* moments;              /* [4][DAD_EV_MOMENTS] */
  int64_t n;                    /* utterances, >= 1 */
  int64_t slabs;                /* slab_off[n] */
  int32_t store_dtype;          /* DAD_STORE_* */
  int32_t use_entropy;          /* USE_ENTROPY_IN_SCORE */
  int32_t precision;            /* DAD_PREC_FP32 (exact-f32 MFMA, the reference's eval arithmetic) or
                                   DAD_PREC_FP16 (rows and W1 rounded to fp16, fp32 accumulation) */
  int32_t reserved;
} dad_eval_args;
/* workspace bytes of dad_eval_split (0 for an unsupported n / slabs); no initialisation needed */
size_t dad_eval_workspace_bytes(int64_t n, int64_t slabs, int precision, int with_teacher);
/* DAD_E_ARG: a required pointer is NULL or a dtype / precision value is unknown; DAD_E_SHAPE: n < 1 or
 * slabs outside [0, n * 2^26]; DAD_E_UNSUPPORTED: DAD_PREC_BF16. */
int dad_eval_split(const dad_eval_args* args, void* workspace, void* stream);

/* --- windows of a split: emotion over time, store-fed (csrc/eval_windows.hip) -------------
 * dad_eval_split answers once per utterance.  dad_eval_windows classifies every sliding window, or every
 * prefix, of every utterance of a split in one pass over the store: the encoder is frame-wise, so a window's
 * embedding is a partial sum of the per-frame rows relu(W1 x_t + b1) that the split evaluator already computes.
 * By definition a window's outputs are SSRLModel.predict / get_embeddings (I/model.py:225-265) on the
 * utterance's features cropped to the window.
 *
 * Utterance i has L = lens[i] frames; the hop is h = hop >= 1 frames and the span m = span >= 1 hops.
 *   S = ceil(L / h) hop-segments; segment s is frames [s h, min((s + 1) h, L)).
 *   DAD_WIN_SLIDING  J = 0 if L = 0, else max(1, S - m + 1); window j is frames [j h, min((j + m) h, L)).  The
 *                    last window ends at L; an utterance shorter than m h has one window, itself.
 *   DAD_WIN_PREFIX   J = S; window j is frames [0, min((j + 1) h, L)).  span must be 1 (DAD_E_ARG otherwise).
 *                    The last prefix is the whole utterance.
 * For a window of c frames: embedding = (sum over its frames of relu(W1 x_t + b1)) / c; logits, softmax
 * probabilities, certainty score and first-maximum argmax by dad_predict_head's / dad_eval_split's arithmetic.
 * Windows are laid out ragged: win_off[n + 1] is the exclusive prefix of J and `windows` = win_off[n].
 *
 * The encoder sums the rows per piece: a maximal run of frames inside one 32-frame slab and one hop-segment.
 * An utterance's pieces, in frame order, are cut at every multiple of 32 and of h below L (a slab holds at most
 * min(32, ceil(32 / h) + 1) of them); piece_off[n + 1] is the exclusive prefix of their number,
 * ceil(L / 32) + ceil(L / h) - ceil(L / lcm(32, h)), and `pieces` = piece_off[n].  A window's sum is the
 * left-to-right fp32 sum of its pieces from 0, as dad_eval_split sums slab partials; SLIDING re-sums every
 * window's pieces (no subtraction of running sums), so for h % 32 == 0 the last PREFIX window equals
 * dad_eval_split's emb / logits / pred bit for bit, and SLIDING (h, 1) and PREFIX (h, 1) agree bit for bit on
 * window 0.  Both prefixes are pure host functions of (lens, hop, span, mode).  win_off_host is the HOST copy
 * of win_off: the entry point reads its first and last entries to hold `windows` to it before anything is
 * launched (DAD_E_ARG).  An utterance whose device entries disagree with its length is treated as J = 0.
 * windows and pieces must be below 2^31 (DAD_E_SHAPE).
 *
 * Per-utterance outputs; for an utterance with J = 0 every integer output is -1 and mean_probs is 0:
 *   mean_probs [n][4]  the window probabilities summed in window order in fp32, / J
 *   mean_pred [n]      first-maximum argmax of mean_probs
 *   vote_pred [n]      the class most windows predict, ties to the lowest class index
 *   last_pred [n]      w_pred of the last window
 *   settle [n]         the smallest j such that every window j' >= j predicts last_pred
 *   switches [n]       the number of j >= 1 with w_pred[j] != w_pred[j - 1]
 * Result block: result[DAD_EW_SLOTS] int64 (exact). */
#define DAD_WIN_SLIDING 0
#define DAD_WIN_PREFIX 1
#define DAD_EW_CONF_MEAN 0      /* [4][4] row = label, column = mean_pred, over labelled utterances with J > 0 */
#define DAD_EW_CONF_VOTE 16     /* the same for vote_pred */
#define DAD_EW_CONF_LAST 32     /* the same for last_pred */
#define DAD_EW_N 48             /* n */
#define DAD_EW_N_LABELLED 49    /* utterances with a label in [0, 4) */
#define DAD_EW_N_EMPTY 50       /* utterances with J = 0 */
#define DAD_EW_N_WINDOWS 51     /* windows */
#define DAD_EW_N_NONFINITE 52   /* windows with a logit that is not finite */
#define DAD_EW_SETTLE_SUM 53    /* over utterances with J > 0: sum of settle */
#define DAD_EW_SWITCHES_SUM 54  /* sum of switches */
#define DAD_EW_SETTLE_FRAMES_SUM 55 /* sum of the exclusive end frame of window `settle` */
#define DAD_EW_CURVE 64         /* curve slots: window index j < 64 (56..63 reserved, written 0) */
#define DAD_EW_REACHED 64       /* [64] labelled utterances with J > j */
#define DAD_EW_CORRECT 128      /* [64] those of them with w_pred[j] == label */
#define DAD_EW_CARRIED 192      /* [64] labelled utterances with J > 0 whose w_pred[min(j, J - 1)] == label */
#define DAD_EW_SLOTS 256
/* Rows as dad_eval_args (store, rows, lens, labels, slab_off, slabs).  One network per call: params is the
 * student's or the teacher's flat vector.  Optional outputs: NULL = not written.  Enqueue only, no allocation,
 * no device read on the host, no floating-point atomics: two calls on the same inputs write the same bits. */
typedef struct dad_window_args {
  const void* store;            /* [frames][768], dtype store_dtype */
  const int64_t* rows;          /* [n] store row of frame 0 */
  const int32_t* lens;          /* [n] frames */
  const int64_t* labels;        /* [n] or NULL */
  const int32_t* slab_off;      /* [n + 1] exclusive prefix of ceil(lens / 32) */
  const float* params;          /* [DAD_NPARAM] flat [W1|b1|W2|b2] */
  const int32_t* win_off;       /* [n + 1] device: exclusive prefix of J */
  const int32_t* piece_off;     /* [n + 1] device: exclusive prefix of the piece counts */
  const int32_t* win_off_host;  /* [n + 1] HOST copy of win_off */
  float* w_emb;                 /* [windows][256] */
  float* w_logits;              /* [windows][4] */
  float* w_probs;               /* [windows][4] */
  float* w_score;               /* [windows] certainty score (dad_predict_head's) */
  int64_t* w_pred;              /* [windows] first-maximum argmax */
  float* mean_probs;            /* [n][4] */
  int64_t* mean_pred;           /* [n] */
  int64_t* vote_pred;           /* [n] */
  int64_t* last_pred;           /* [n] */
  int32_t* settle;              /* [n] */
  int32_t* switches;            /* [n] */
  int64_t* result;              /* [DAD_EW_SLOTS], required */
  int64_t n;                    /* utterances, >= 1 */
  int64_t slabs;                /* slab_off[n] */
  int64_t windows;              /* win_off[n] */
  int64_t pieces;               /* piece_off[n] */
  int32_t hop;                  /* frames, >= 1 */
  int32_t span;                 /* hops, >= 1 */
  int32_t mode;                 /* DAD_WIN_* */
  int32_t store_dtype;          /* DAD_STORE_* */
  int32_t use_entropy;          /* USE_ENTROPY_IN_SCORE */
  int32_t precision;            /* DAD_PREC_FP32 (exact-f32 MFMA) or DAD_PREC_FP16 (rows and W1 rounded to fp16) */
} dad_window_args;
/* workspace bytes of dad_eval_windows (0 for unsupported sizes); no initialisation needed */
size_t dad_eval_windows_workspace_bytes(int64_t n, int64_t slabs, int64_t windows, int64_t pieces, int precision);
/* DAD_E_ARG: a required pointer is NULL, an unknown dtype / precision / mode, hop < 1, span < 1, PREFIX with
 * span != 1, or windows != win_off_host[n]; DAD_E_SHAPE: n < 1, slabs outside [0, n * 2^26], windows or pieces
 * outside [0, 2^31) or pieces < slabs; DAD_E_UNSUPPORTED: DAD_PREC_BF16.  Nothing is launched on an error. */
int dad_eval_windows(const dad_window_args* args, void* workspace, void* stream);

/* --- noise response of a split: every noise level in one store pass (csrc/eval_noise.hip) ----
 * The train step asks the model to hold its decision under x + std * N (DataAugmentation.weak_augment /
 * strong_augment, I/utils.py:328-350).  dad_eval_noise evaluates a split at K noise levels of ONE draw in one
 * pass over the store.  By definition level k's outputs are SSRLModel.get_embeddings / predict (I/model.py:
 * 225-265) in eval mode on x_t + sigma[k] * n_t over the utterance's lens[i] frames, n_t standard normal.
 *
 * The encoder is frame-wise and linear before its ReLU: W1 (x_t + s n_t) + b1 = W1 x_t + s W1 n_t + b1.  The slab
 * kernel therefore runs two GEMMs per 32-frame slab on one W1 fragment, acc0 = x W1 and acc1 = n W1, and each
 * level is only an epilogue, relu(fma(sigma[k], acc1, acc0) + b1) summed over the slab's valid rows, and a head.
 * The same draw serves every level (common random numbers): the levels of one call differ by sigma only.
 *
 * Noise.  noise == NULL: counter mode.  The normal of (utterance i, frame t, channel d) is a pure function of
 * (seed, draw, i, t, d): dad_normal_pair on a key derived from dad_stream_key(seed, draw, DAD_RNG_EVAL_NOISE), i
 * and t >> 22, at element (t mod 2^22) * 768 + d.  It depends on neither the slab assignment, the launch
 * geometry, the store row nor the other utterances, and no index wraps in 32 bits at any supported size.
 * Otherwise noise is an explicit float [32 * slabs][768]: frame t of utterance i is row 32 * slab_off[i] + t (the
 * slab-aligned layout; rows past an utterance's length are not used).  dad_eval_noise_draws writes the counter
 * mode's normals in that layout (zeros in the unused rows) with the same device functions, so a counter call
 * equals, bit for bit, an explicit call fed the probe's output.
 *
 * Precision.  DAD_PREC_FP32: exact-f32 MFMA for both GEMMs.  DAD_PREC_FP16: the rows, the noise and W1 are each
 * rounded to fp16 (fp32 accumulation); sigma is applied in fp32 in the epilogue in both modes.
 * Bit identities.  fma(0, finite, a) = a, and the k order, the epilogue order and the head are dad_eval_split's:
 * a level with sigma = 0 equals dad_eval_split's emb / logits / probs / score / pred for the same network bit for
 * bit, in both precisions and for the three store types.  Two levels with the same sigma are equal bit for bit;
 * two calls on the same inputs write the same bits (no floating-point atomics).
 *
 * Per-utterance outputs, level-major, all optional (NULL = not written):
 *   emb [K][n][256], logits [K][n][4], probs [K][n][4], score [K][n], pred [K][n]   as dad_eval_split's
 *   drift [K][n]       |e_k - e_0|_2, an fp32 sum in a fixed order
 *   kl [K][n]          sum_c p_0c (log p_0c - log p_kc), 0 log 0 = 0: the per-sample term of the consistency loss
 *                      with level 0 in the teacher's role, from the log-softmax of the two logit rows
 *   break_level [n]    int32, the smallest k >= 1 with pred_k != pred_0, or K
 * Level 0 is the base level those three refer to (callers put sigma[0] = 0 for a clean base; not required).
 * A length-0 utterance (or one whose slab_off entries disagree with its length) has a zero embedding, logits = b2
 * at every level, drift 0, kl 0 and break_level K.
 *
 * Result block: counts[DAD_EN_COUNTS] int64 and sums[DAD_EN_SUMS] double, fixed size for DAD_EN_MAX_LEVELS
 * levels; the slots of unused levels are written 0. */
#define DAD_EN_MAX_LEVELS 8
#define DAD_EN_CONF 0           /* [8][4][4] per level: row = label, column = pred_k (labelled utterances) */
#define DAD_EN_FLIPS 128        /* [8] utterances with pred_k != pred_0, over all n */
#define DAD_EN_SURVIVE 136      /* [8] utterances with break_level > k */
#define DAD_EN_N 144            /* n */
#define DAD_EN_N_LABELLED 145   /* utterances with a label in [0, 4) */
#define DAD_EN_N_SKIPPED 146    /* label outside [0, 4), or labels == NULL (then n) */
#define DAD_EN_N_NONFINITE 147  /* utterances with a logit that is not finite at any level */
#define DAD_EN_LEVELS 148       /* K */
#define DAD_EN_COUNTS 160       /* int64 slots of the counts block (149..159 reserved, written 0) */
/* sums[.][k]: float64 sums over all n of the float32 per-utterance values, in a fixed order (strided per-thread
 * sums and an LDS tree, as dad_eval_split's moments) */
#define DAD_EN_SUM_SCORE 0      /* [8] */
#define DAD_EN_SUM_DRIFT 8      /* [8] */
#define DAD_EN_SUM_KL 16        /* [8] */
#define DAD_EN_SUMS 24
/* Rows as dad_eval_args (store, rows, lens, labels, slab_off, slabs).  One network per call: params is the
 * student's or the teacher's flat vector.  Enqueue only, no allocation, no device read on the host. */
typedef struct dad_noise_args {
  const void* store;            /* [frames][768], dtype store_dtype */
  const int64_t* rows;          /* [n] store row of frame 0 */
  const int32_t* lens;          /* [n] frames */
  const int64_t* labels;        /* [n] or NULL */
  const int32_t* slab_off;      /* [n + 1] exclusive prefix of ceil(lens / 32) */
  const float* params;          /* [DAD_NPARAM] flat [W1|b1|W2|b2] */
  const float* noise;           /* [32 * slabs][768] explicit normals, or NULL: counter mode */
  float* emb;                   /* [K][n][256] */
  float* logits;                /* [K][n][4] */
  float* probs;                 /* [K][n][4] */
  float* score;                 /* [K][n] */
  int64_t* pred;                /* [K][n] */
  float* drift;                 /* [K][n] */
  float* kl;                    /* [K][n] */
  int32_t* break_level;         /* [n] */
  int64_t* counts;              /* [DAD_EN_COUNTS], required */
  double* sums;                 /* [DAD_EN_SUMS], required */
  int64_t n;                    /* utterances, >= 1 */
  int64_t slabs;                /* slab_off[n] */
  uint64_t seed;                /* counter mode: the stream key is dad_stream_key(seed, draw, DAD_RNG_EVAL_NOISE) */
  uint64_t draw;
  float sigma[DAD_EN_MAX_LEVELS]; /* [levels] host values, each finite and >= 0 */
  int32_t levels;               /* K in [1, DAD_EN_MAX_LEVELS] */
  int32_t store_dtype;          /* DAD_STORE_* */
  int32_t use_entropy;          /* USE_ENTROPY_IN_SCORE */
  int32_t precision;            /* DAD_PREC_FP32 or DAD_PREC_FP16 */
} dad_noise_args;
/* workspace bytes of dad_eval_noise: slabs * levels * 1 KB of slab partials plus per-utterance words (0 for
 * unsupported sizes); no initialisation needed */
size_t dad_eval_noise_workspace_bytes(int64_t n, int64_t slabs, int levels, int precision);
/* Checked on the host before anything is launched.  DAD_E_ARG: a required pointer is NULL, levels outside [1, 8],
 * a sigma negative or not finite, an unknown dtype / precision; DAD_E_SHAPE: n < 1, slabs outside [0, n * 2^26],
 * or slabs * levels * 256 >= 2^31; DAD_E_UNSUPPORTED: DAD_PREC_BF16. */
int dad_eval_noise(const dad_noise_args* args, void* workspace, void* stream);
/* The probe: the counter mode's normals of (args->seed, args->draw) for args->lens / slab_off / n / slabs, as the
 * explicit layout out [32 * slabs][768] (device).  Reads no other field.  DAD_E_ARG: args, out, lens or slab_off
 * NULL; DAD_E_SHAPE as above (levels taken as 1). */
int dad_eval_noise_draws(const dad_noise_args* args, float* out, void* stream);

/* --- several networks on one split: up to 8 checkpoints in one store pass (csrc/eval_models.hip) ----
 * The reference compares networks on the same split everywhere around its train step: the fold checkpoints
 * (best_model_fold_k.ckpt), the ablation runners' BEST checkpoints, inference.py's weights one after another, the
 * student / teacher pair.  dad_eval_models evaluates K networks on a split in one call and leaves what such a
 * comparison reads in one result block: who is better, whether the difference is more than chance (McNemar's two
 * cells), how often two networks disagree, and what their ensemble and their majority vote would score.
 *
 * Members.  m < K is model k = m; m = K is the mean ensemble; m = K + 1 is the vote.
 * Per model k: emb / logits / probs / score / pred [k][n] are dad_eval_split's for student = models[k], bit for bit,
 * in both precisions and for the three store types (the same loaders, k order, epilogue order and head; the slab
 * kernel runs two consecutive slab jobs per wave on one W1 fragment, which changes no accumulator's chain).  An
 * utterance of length 0, or one whose slab_off entries disagree with its length, has a zero embedding and logits =
 * b2 of every model.
 * Mean ensemble: w^_k = (float)(weight[k] / sum_j weight[j]), the quotient in double on the host (sum in k order);
 *   ens_probs[c] is the fp32 chain e = 0; e = fmaf(w^_k, p_k[c], e) for k = 0 .. K - 1; ens_pred its first-maximum
 *   argmax; ens_score the head's certainty formula on ens_probs (max_c e_c * (1 - H_2(e + 1e-8) / 2), or max_c e_c
 *   without use_entropy).  With K = 1, ens_probs equals probs[0] bit for bit.
 * Vote: votes[u][c] is the number of models with pred_k = c; vote_pred is the class with most votes, ties to the
 *   lowest class index (dad_knn_vote's and dad_eval_windows' rule).  n_correct[u] is the number of models that are
 *   right, or -1 for an utterance without a label in [0, 4).
 *
 * counts[DAD_EM_COUNTS] int64: the layout does not depend on K; entries of unused members are written 0. */
#define DAD_EM_MAX_MODELS 8
#define DAD_EM_MEMBERS 10       /* K models, then the mean ensemble (index K), then the vote (index K + 1) */
#define DAD_EM_CONF 0           /* [10][4][4] per member: row = label, column = prediction (labelled utterances) */
#define DAD_EM_DISAGREE 160     /* [10][10] pred_a != pred_b, over all n utterances */
#define DAD_EM_ONLY 260         /* [10][10] labelled utterances where a is right and b is wrong; the diagonal is a's
                                   correct count; ONLY[a][b] and ONLY[b][a] are McNemar's two cells */
#define DAD_EM_HIST 360         /* [9] labelled utterances by how many of the K models are right */
#define DAD_EM_N 369            /* n */
#define DAD_EM_N_LABELLED 370   /* utterances with a label in [0, 4) */
#define DAD_EM_N_SKIPPED 371    /* label outside [0, 4), or labels == NULL (then n) */
#define DAD_EM_NONFINITE 372    /* [8] per model: utterances with a logit that is not finite */
#define DAD_EM_K 380            /* K */
#define DAD_EM_COUNTS 384       /* int64 slots of the counts block (381..383 reserved, written 0) */
/* sums[DAD_EM_SUMS] double, [quantity][member], members m <= K (the vote has no probabilities; its slots and those
 * of unused members are written 0).  Every term is computed in double from the float32 probabilities (the score from
 * the float32 score) and summed in a fixed order (strided per-thread sums and an LDS tree, as dad_eval_split's
 * moments): no floating-point atomics, two calls give the same bits. */
#define DAD_EM_SUM_SCORE 0      /* [10] certainty score, over all n */
#define DAD_EM_SUM_ENTROPY 10   /* [10] -sum_c p_c ln p_c (0 ln 0 = 0), over all n */
#define DAD_EM_SUM_NLL 20       /* [10] -ln p_y, over labelled utterances */
#define DAD_EM_SUM_BRIER 30     /* [10] sum_c (p_c - [y = c])^2, over labelled utterances */
#define DAD_EM_SUMS 40
/* Rows as dad_eval_args (store, rows, lens, labels, slab_off, slabs).  Enqueue only, no allocation, no device read
 * on the host.  Per-model outputs are model-major (dad_eval_noise's [K][n] layout); every output but counts and sums
 * is optional (NULL = not written). */
typedef struct dad_models_args {
  const void* store;            /* [frames][768], dtype store_dtype */
  const int64_t* rows;          /* [n] store row of frame 0 */
  const int32_t* lens;          /* [n] frames */
  const int64_t* labels;        /* [n] or NULL */
  const int32_t* slab_off;      /* [n + 1] exclusive prefix of ceil(lens / 32) */
  int64_t n;                    /* utterances, >= 1 */
  int64_t slabs;                /* slab_off[n] */
  int32_t store_dtype;          /* DAD_STORE_* */
  int32_t use_entropy;          /* USE_ENTROPY_IN_SCORE */
  int32_t precision;            /* DAD_PREC_FP32 or DAD_PREC_FP16 */
  int32_t reserved0;
  const float* models[DAD_EM_MAX_MODELS];   /* device, flat [W1|b1|W2|b2]; entries >= K ignored; may repeat */
  float weight[DAD_EM_MAX_MODELS];  /* [K] host values, the ensemble weights: finite, >= 0, sum > 0 */
  int32_t K;                    /* models, in [1, DAD_EM_MAX_MODELS] */
  int32_t reserved1;
  /* per-model outputs */
  float* emb;                   /* [K][n][256] */
  float* logits;                /* [K][n][4] */
  float* probs;                 /* [K][n][4] */
  float* score;                 /* [K][n] */
  int64_t* pred;                /* [K][n] */
  /* per-utterance outputs */
  float* ens_probs;             /* [n][4] */
  float* ens_score;             /* [n] */
  int64_t* ens_pred;            /* [n] */
  int64_t* vote_pred;           /* [n] */
  int32_t* votes;               /* [n][4] */
  int32_t* n_correct;           /* [n], -1 unlabelled */
  int64_t* counts;              /* [DAD_EM_COUNTS], required */
  double* sums;                 /* [DAD_EM_SUMS], required */
} dad_models_args;
/* workspace bytes of dad_eval_models: K * slabs * 1 KB of slab partials, per-utterance words and, in DAD_PREC_FP16,
 * K fp16 copies of W1 (0 for unsupported sizes or K); no initialisation needed */
size_t dad_eval_models_workspace_bytes(int64_t n, int64_t slabs, int K, int precision);
/* Checked on the host before anything is launched.  DAD_E_ARG: a required pointer is NULL, K outside [1, 8], a
 * models[k] (k < K) NULL, a weight negative or not finite, sum of the weights 0, an unknown dtype / precision;
 * DAD_E_SHAPE: n < 1, slabs outside [0, n * 2^26], or K * slabs * 256 >= 2^31; DAD_E_UNSUPPORTED: DAD_PREC_BF16. */
int dad_eval_models(const dad_models_args* args, void* workspace, void* stream);

/* --- input gradients of a split: the worst-case direction, store-fed (csrc/input_grad.hip) ----
 * dad_eval_noise measures a split under RANDOM noise.  dad_input_grad gives the direction of the WORST perturbation
 * of the same size: the vector-Jacobian product of the eval-mode forward (SSRLModel.predict, I/model.py:225-245)
 * with respect to the stored rows, which the reference's autograd never forms (its inputs do not require grad).
 *
 * Definition.  For utterance u with len frames x_t, an optional perturbation delta_t and the caller's logit
 * cotangent dz_u[4]:
 *   pre_tj = W1[j] . (x_t + delta_t) + b1[j],   m_tj = pre_tj > 0   (torch's ReLU': 0 at 0)
 *   s_u[j] = sum_c W2[c][j] dz_u[c],            g_u = s_u / max(len, 1)
 *   G_t[d] = sum_j m_tj g_u[j] W1[j][d]
 *   step_t[d] = clamp(delta_t[d] + alpha sgn(G_t[d]), -radius, +radius),   sgn(0) = 0, delta = 0 when NULL
 * With dz = softmax(z) - onehot(target), G is the gradient of PLAIN cross-entropy of the utterance with respect to
 * its frames (not of the trainer's label-smoothed loss), the step with delta = NULL is FGSM (Goodfellow et al. 2015)
 * and iterating it with delta_out fed back as delta_in is PGD (Madry et al. 2018).
 *
 * Layout.  delta_in, grad and delta_out are float [32 * slabs][768] in dad_eval_noise's explicit layout: frame t of
 * utterance i is row 32 * slab_off[i] + t, so a delta_out is a `noise` of dad_eval_noise as it stands; frame_l1 is
 * float [32 * slabs] with sum_d |G_t[d]| (fp32, a fixed order) in the same rows.  Rows past an utterance's length
 * are written 0 in every output, so no buffer needs initialising; a length-0 utterance owns no slab and writes
 * nothing.  All three outputs are optional (NULL = not written).  delta_out may be delta_in itself: every element is
 * read and written by the same lane.  A G element that is not finite takes step 0 and is counted.
 *
 * Precision.  DAD_PREC_FP32: exact-f32 MFMA for both GEMMs; g_u in fp32 (one product and three fmas over c, then the
 * division).  DAD_PREC_FP16: x + delta is summed in f32 and rounded once to fp16, W1 is rounded to fp16 (a row-major
 * and a transposed copy in the workspace), and the backward A operand is m (.) (c_u s_u) rounded to fp16 with c_u the
 * power of two that puts max_j |s_u[j]| into [2^14, 2^15) (g_u of a long utterance would fall into fp16's subnormals
 * otherwise); fp32 accumulation, and 1 / c_u and 1 / max(len, 1) are applied in fp32 after the GEMM.
 * Bit identities.  With delta_in == NULL the forward accumulators hold dad_eval_split's bits (the same loaders and
 * k order); delta_in == NULL equals a delta_in of zeros; the result depends on neither the order of the utterances
 * nor the slab-to-workgroup assignment; two calls on the same inputs write the same bits (integer atomics only). */
#define DAD_IG_FRAMES 0         /* frames processed (the sum of lens) */
#define DAD_IG_NONFINITE 1      /* elements of G, over those frames, that are not finite */
#define DAD_IG_ZERO 2           /* elements of G, over those frames, that equal 0 */
#define DAD_IG_COUNTS 4         /* int64 slots of the counts block (3 reserved, written 0) */
/* Rows as dad_eval_args (store, rows, lens, slab_off, slabs).  One network per call.  Enqueue only, no allocation,
 * no device read on the host; the call itself zeroes counts. */
typedef struct dad_input_grad_args {
  const void* store;            /* [frames][768], dtype store_dtype */
  const int64_t* rows;          /* [n] store row of frame 0 */
  const int32_t* lens;          /* [n] frames */
  const int32_t* slab_off;      /* [n + 1] exclusive prefix of ceil(lens / 32) */
  const float* params;          /* [DAD_NPARAM] flat [W1|b1|W2|b2] */
  const float* dz;              /* [n][4] logit cotangents, required */
  const float* delta_in;        /* [32 * slabs][768] or NULL: no perturbation */
  float* grad;                  /* [32 * slabs][768] */
  float* delta_out;             /* [32 * slabs][768]; may alias delta_in */
  float* frame_l1;              /* [32 * slabs] */
  int64_t* counts;              /* [DAD_IG_COUNTS], required */
  int64_t n;                    /* utterances, >= 1 */
  int64_t slabs;                /* slab_off[n] */
  float alpha;                  /* step size, finite */
  float radius;                 /* clamp radius, >= 0; INFINITY = no clamp */
  int32_t store_dtype;          /* DAD_STORE_* */
  int32_t precision;            /* DAD_PREC_FP32 or DAD_PREC_FP16 */
} dad_input_grad_args;
/* workspace bytes of dad_input_grad: the two fp16 copies of W1 in DAD_PREC_FP16, one aligned unit otherwise (0 for
 * unsupported sizes); no initialisation needed */
size_t dad_input_grad_workspace_bytes(int64_t n, int64_t slabs, int precision);
/* Checked on the host before anything is launched.  DAD_E_ARG: args, workspace or a required pointer is NULL, an
 * unknown dtype / precision, alpha not finite, radius negative or NaN; DAD_E_SHAPE: n < 1 or slabs outside
 * [0, n * 2^26]; DAD_E_UNSUPPORTED: DAD_PREC_BF16. */
int dad_input_grad(const dad_input_grad_args* args, void* workspace, void* stream);

/* --- attributions of a split: exact integrated gradients, store-fed (csrc/attribution.hip) ----
 * dad_input_grad gives the LOCAL gradient.  In a ReLU network that is not an attribution: it sums to nothing, and
 * gradient x input reads the wrong side of every unit that switches between the baseline and the input.  Integrated
 * gradients (Sundararajan et al. 2017) along the straight path x' -> x_t sums to the logit difference against the
 * baseline, and for this network it needs no path sampling: the pre-activation is affine in the path parameter, so
 * the path integral of ReLU' is an interval length with a closed form.
 *
 * Definition.  For utterance u with len frames x_t, a baseline row x' (768 floats, one per call, zeros when NULL)
 * and the caller's logit cotangent dz_u[4], HELD FIXED along the path (the attributed quantity is F = dz_u . z, e.g.
 * one logit or a margin; a cotangent that changes along the path, such as a log-probability's, needs quadrature and
 * is out of scope):
 *   p0_j   = W1[j] . x' + b1[j]                     (per call, 256 values)
 *   a_tj   = W1[j] . (x_t - x'),   p1_tj = p0_j + a_tj
 *   l_tj   = |{alpha in [0, 1] : p0_j + alpha a_tj > 0}|
 *          = 1                      p0 > 0,  p1 > 0
 *          = 0                      p0 <= 0, p1 <= 0
 *          = p1 / (p1 - p0)         p0 <= 0 < p1
 *          = p0 / (p0 - p1)         p1 <= 0 < p0
 *   g_u    = W2^T dz_u / max(len, 1)                (dad_input_grad's g_u, the same order of operations)
 *   attr_t[d]      = (x_t[d] - x'[d]) sum_j l_tj g_u[j] W1[j][d]
 *   frame_attr_t   = sum_j g_u[j] (ReLU(p1_tj) - ReLU(p0_j))        ( = sum_d attr_t[d] in exact arithmetic )
 *   chan_attr_u[d] = sum_t attr_t[d],     utt_total_u = sum_t frame_attr_t
 * l_tj a_tj = ReLU(p1_tj) - ReLU(p0_j) in all four cases, hence sum_d attr_t[d] = frame_attr_t, hence completeness:
 * utt_total_u = dz_u . (z(x) - z(x')) with z(x') = W2 ReLU(p0) + b2.
 *
 * Arithmetic.  a = W1 x comes from the stored rows in place; W1 x' (a prologue launch, one wave per hidden unit,
 * a fixed order) is subtracted in fp32 behind the GEMM, p1 = p0 + (W1 x - W1 x').  frame_attr is one fma per hidden
 * unit in a fixed order and needs no second GEMM: with attr == NULL and chan_attr == NULL (frame-only mode) the call
 * costs one forward pass.  Otherwise the data-gradient GEMM runs on the float coefficients l_tj g_u[j], which stay in
 * registers between the two GEMMs.  DAD_PREC_FP32: exact-f32 MFMA for both.  DAD_PREC_FP16: the rows, W1 and (for
 * p0 and W1 x') the baseline are rounded to fp16, fp32 accumulation; the coefficient l_tj (c_u s_u[j]) is formed in
 * fp32 and rounded once to fp16 with dad_input_grad's power of two c_u, and 1 / c_u and 1 / max(len, 1) are applied in
 * fp32 after the GEMM (l <= 1, so no coefficient overflows); the factor x_t[d] - x'[d] is the fp32 difference of the
 * widened stored value and the unrounded baseline in both precisions.
 *
 * Layout.  attr is float [32 * slabs][768] and frame_attr float [32 * slabs] in dad_eval_noise's explicit layout;
 * chan_attr is [n][768] (slab partials in the workspace, then a per-utterance sum in slab order) and utt_total [n]
 * (a fixed order).  Every output but counts is optional.  Rows past an utterance's length are written 0, so no
 * buffer needs initialising; a length-0 utterance owns no slab and gets utt_total 0 and a zero chan_attr row.  An
 * attr element that is not finite is written 0 (and enters chan_attr as 0) and is counted.
 *
 * Bit identities.  baseline == NULL equals a baseline of zeros; frame_attr and utt_total are the same bits in
 * frame-only and full mode; the result of an utterance depends on neither the order of the utterances nor the
 * slab-to-workgroup assignment; two calls on the same inputs write the same bits (integer atomics only). */
#define DAD_AT_FRAMES 0         /* frames processed (the sum of lens) */
#define DAD_AT_NONFINITE 1      /* attr elements, over those frames, that were not finite (written 0); 0 in frame-only mode */
#define DAD_AT_CROSS 2          /* (t, j) pairs, over those frames, whose path crosses zero (0 < l < 1 by case) */
#define DAD_AT_ONE 3            /* (t, j) pairs with l = 1 */
#define DAD_AT_COUNTS 4         /* int64 slots of the counts block */
/* Rows as dad_eval_args (store, rows, lens, slab_off, slabs).  One network per call.  Enqueue only, no allocation,
 * no device read on the host; the call itself zeroes counts. */
typedef struct dad_attribution_args {
  const void* store;            /* [frames][768], dtype store_dtype */
  const int64_t* rows;          /* [n] store row of frame 0 */
  const int32_t* lens;          /* [n] frames */
  const int32_t* slab_off;      /* [n + 1] exclusive prefix of ceil(lens / 32) */
  const float* params;          /* [DAD_NPARAM] flat [W1|b1|W2|b2] */
  const float* dz;              /* [n][4] logit cotangents, required */
  const float* baseline;        /* [768] or NULL: zeros */
  float* attr;                  /* [32 * slabs][768] */
  float* frame_attr;            /* [32 * slabs] */
  float* chan_attr;             /* [n][768] */
  float* utt_total;             /* [n] */
  int64_t* counts;              /* [DAD_AT_COUNTS], required */
  int64_t n;                    /* utterances, >= 1 */
  int64_t slabs;                /* slab_off[n] */
  int32_t store_dtype;          /* DAD_STORE_* */
  int32_t precision;            /* DAD_PREC_FP32 or DAD_PREC_FP16 */
} dad_attribution_args;
/* workspace bytes that hold for every mode: p0, W1 x', x', the slab totals, the slab channel partials
 * (slabs * 3 KB) and in DAD_PREC_FP16 the two fp16 copies of W1 (0 for unsupported sizes); no initialisation needed */
size_t dad_attribution_workspace_bytes(int64_t n, int64_t slabs, int precision);
/* Checked on the host before anything is launched.  DAD_E_ARG: args, workspace or a required pointer is NULL, or an
 * unknown dtype / precision; DAD_E_SHAPE: n < 1 or slabs outside [0, n * 2^26]; DAD_E_UNSUPPORTED: DAD_PREC_BF16. */
int dad_attribution(const dad_attribution_args* args, void* workspace, void* stream);
/* Host-only: what dad_attribution would do with args (the same checks and codes; no workspace needed). */
#define DAD_AT_PLAN_MODE 0      /* 0: frame-only (one GEMM), 1: full (attr or chan_attr given: two GEMMs) */
#define DAD_AT_PLAN_BYTES 1     /* the prefix of the workspace this call touches */
#define DAD_AT_PLAN_LAUNCHES 2  /* kernel launches */
#define DAD_AT_PLAN_KERNEL 3    /* the slab kernel's instance: 4 * store_dtype + 2 * (FP16) + (full) */
#define DAD_AT_PLAN_SLOTS 4
int dad_attribution_plan(const dad_attribution_args* args, int64_t* out);

/* --- class separation of a split's embeddings (csrc/cluster.hip) -------------------------
 * calculate_cluster_metrics (I/iemocap_plot_tsne.py:390-398): scikit-learn's silhouette_score and
 * calinski_harabasz_score of emb [n][256] (dad_eval_split's emb / t_emb) under labels [n], whose
 * values generate_analysis_report (I/iemocap_plot_tsne.py:400-470) writes into `cluster_analysis`.
 * Only rows with a label in [0, 4) take part (m of them, k classes present, n_c per class).  With
 * d(i, j) the Euclidean distance (d(i, i) = 0): a(i) = sum of d(i, j) over the other rows of i's class
 * / (n_c - 1); b(i) = min over the other present classes of the mean d(i, j) to their rows;
 * s(i) = (b - a) / max(a, b), 0 when n_c = 1 or max(a, b) = 0; silhouette = mean s(i).
 * CH = (B / (k - 1)) / (W / (m - k)), B = sum_c n_c |mu_c - mu|^2, W = sum_i |x_i - mu_{y_i}|^2, 1.0 when
 * W = 0.  Both are defined for 2 <= k <= m - 1 only; otherwise (scikit-learn raises, the reference
 * reports (0.0, 0.0)) DAD_CM_VALID is 0, both scores are 0.0 and every s(i) is 0.
 * The distances come from a Gram pass on the fp32 matrix cores, d = sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j,
 * 0)) on rows centred on the labelled rows' mean (a shift changes no distance and removes the common
 * post-ReLU offset from the cancellation); the per-row class sums are added in a fixed order (no floating-point atomics), so two calls on
 * the same inputs write bit-identical outputs.  Rows past n are never read.
 * out [DAD_CM_SLOTS] doubles (device); sil [n] (device, may be NULL) receives s(i), 0 for an unlabelled row. */
#define DAD_CM_SILHOUETTE 0
#define DAD_CM_CH 1
#define DAD_CM_VALID 2          /* 1.0 / 0.0 */
#define DAD_CM_M 3              /* labelled rows */
#define DAD_CM_K 4              /* classes present */
#define DAD_CM_COUNTS 5         /* [4] n_c */
#define DAD_CM_SIL_CLASS 9      /* [4] mean s(i) of the class (0 for an absent class) */
#define DAD_CM_W 13
#define DAD_CM_B 14
#define DAD_CM_NONFINITE 15     /* labelled rows with a non-finite component (the scores are then meaningless) */
#define DAD_CM_SLOTS 16
#define DAD_CM_MAX_N 65536      /* largest n */
#define DAD_CM_TILE 64          /* rows / columns of a tile of the pairwise pass */
#define DAD_CM_MAX_CHUNKS 16    /* most column chunks a row tile is split into */
/* workspace bytes of dad_cluster_metrics (0 for an unsupported n); no initialisation needed */
size_t dad_cluster_workspace_bytes(int64_t n);
/* DAD_E_ARG: emb, labels, out or workspace is NULL; DAD_E_SHAPE: n < 1 or n > DAD_CM_MAX_N. */
int dad_cluster_metrics(const float* emb, const int64_t* labels, int64_t n, double* out, float* sil,
                        void* workspace, void* stream);
/* The grid of the pairwise pass for n rows on a device of `cus` compute units: ceil(n / 64) row tiles,
 * each split into `chunks` runs of tiles_per_chunk column tiles (the last may be shorter, none is
 * empty), chunks <= min(row tiles, DAD_CM_MAX_CHUNKS).  Host only. */
int dad_cluster_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk);
/* dad_cluster_metrics with the chunk count asked for (clamped as dad_cluster_plan clamps it; <= 0: the
 * plan's), for tests of the chunked summation at small n. */
int dad_cluster_metrics_chunked(const float* emb, const int64_t* labels, int64_t n, double* out, float* sil,
                                int chunks, void* workspace, void* stream);

/* --- exact t-SNE of a split's embeddings (csrc/tsne.hip) ----------------------------------
 * run_tsne (I/iemocap_plot_tsne.py:310-323): scikit-learn 1.7.2's TSNE(n_components=2, method='exact') on
 * emb [n][256] (dad_eval_split's emb / t_emb), in the three stages of sklearn/manifold/_t_sne.py.  Every call
 * only enqueues on `stream`, uses no floating-point atomics and takes every sum in a fixed order, so two
 * calls on the same inputs write bit-identical outputs.  One workspace of dad_tsne_workspace_bytes(n) serves
 * all three; it needs no initialisation.  2 <= n <= DAD_TS_MAX_N.
 *
 * P is [n][DAD_TS_LD(n)] floats (n rounded up to the tile; a 1 GiB matrix at DAD_TS_MAX_N): dense, bit-symmetric
 * (P_ij and P_ji are the same bits), P_ii = 0; the calls below never use a padding column's value.
 *
 * dad_tsne_affinities = _joint_probabilities.  D_ij = max(|a_i|^2 + |a_j|^2 - 2 a_i.a_j, 0) on the fp32 matrix
 * cores, a = the rows minus their fp32 mean, |a_i|^2 the diagonal of the same Gram block (D_ii and the distance of
 * duplicate rows are exactly 0) -- the distances of dad_cluster_metrics, squared.  Per row, _binary_search_perplexity
 * in double on the fp32 distances: beta from 1, doubled / halved until bracketed, then bisected, at most 100 steps,
 * until |H - log(perplexity)| <= 1e-5, H = log(sum_j e^(-beta D_ij)) + beta sum_j D_ij c_ij over j != i, a sum of 0
 * replaced by 1e-8; c_ij = e^(-beta D_ij) / sum.  Then P_ij = max((c_ij + c_ji) / max(sum, eps), eps), sum over all
 * i != j in double, eps = 2.220446049250313e-16.  beta [n] doubles (device, may be NULL) receives each row's beta.
 * A row of emb with a non-finite component is counted into the int32 at word DAD_TS_WS_NONFINITE of the workspace
 * (P is then meaningless).  DAD_E_SHAPE: n < 2 or n > DAD_TS_MAX_N; DAD_E_ARG: emb, P or workspace is NULL, or
 * perplexity not in (0, n) (scikit-learn's rule). */
#define DAD_TS_MAX_N 16384      /* largest n */
#define DAD_TS_TILE 64          /* rows / columns of a tile; P's row stride is a multiple of it */
#define DAD_TS_LD(n) (((n) + DAD_TS_TILE - 1) / DAD_TS_TILE * DAD_TS_TILE)
#define DAD_TS_MAX_CHUNKS 32    /* most column chunks a row tile is split into */
#define DAD_TS_WS_NONFINITE 0   /* int32 word of the workspace: rows with a non-finite component (dad_tsne_affinities) */
/* workspace bytes of the three calls (0 for an unsupported n) */
size_t dad_tsne_workspace_bytes(int64_t n);
int dad_tsne_affinities(const float* emb, int64_t n, double perplexity, float* P, double* beta, void* workspace,
                        void* stream);
/* dad_tsne_gradient = _kl_divergence with one degree of freedom, at Y [n][2] with p = exaggeration * P:
 *   w_ij = 1 / (1 + |y_i - y_j|^2)  (from the differences, so coincident points give exactly 1),  Z = sum_{i != j} w_ij,
 *   KL = sum_{i != j} p_ij (log p_ij - log w_ij) + log Z sum p_ij,
 *   grad_i = 4 (sum_j p_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z)        -> grad [n][2] floats.
 * scikit-learn also clamps Q = max(w / Z, eps); the device does not (the clamp acts only where w n^2 < 2.2e-16 Z,
 * an embedding some 1e7 times wider than its typical neighbour distance).  The per-row force sums are fp32; Z, KL and
 * the gradient norm are reduced in double.  out: DAD_TS_SLOTS doubles (device). */
#define DAD_TS_Z 0
#define DAD_TS_KL 1             /* the error; after dad_tsne_run scikit-learn's kl_divergence_ */
#define DAD_TS_GRAD_NORM 2      /* |grad| (dad_tsne_run: of the last iteration's gradient times its gains) */
#define DAD_TS_N_ITER 3         /* dad_tsne_run: scikit-learn's n_iter_ (-1 until the run ends) */
#define DAD_TS_N_CHECKS 4       /* dad_tsne_run: records written to history */
#define DAD_TS_SLOTS 8
/* DAD_E_ARG: a NULL pointer or exaggeration <= 0; DAD_E_SHAPE: n. */
int dad_tsne_gradient(const float* P, int64_t n, const float* Y, double exaggeration, double* out, float* grad,
                      void* workspace, void* stream);
/* The grid of the n x n pass for n rows on a device of `cus` compute units: ceil(n / 64) row tiles, each split
 * into `chunks` runs of tiles_per_chunk column tiles (the last may be shorter, none is empty), chunks <= min(row
 * tiles, DAD_TS_MAX_CHUNKS).  Host only. */
int dad_tsne_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk);
/* dad_tsne_gradient with the chunk count asked for (clamped as dad_tsne_plan clamps it; <= 0: the plan's),
 * for tests of the chunked summation at small n. */
int dad_tsne_gradient_chunked(const float* P, int64_t n, const float* Y, double exaggeration, double* out,
                              float* grad, int chunks, void* workspace, void* stream);
/* dad_tsne_run = TSNE._tsne / _gradient_descent from Y (the initial embedding on entry, the result on exit):
 * min(250, max_iter) exploration iterations at momentum 0.5 on early_exaggeration * P, then momentum 0.8 on P up to
 * max_iter; per element gains += 0.2 where update * grad < 0, otherwise gains *= 0.8, floor 0.01; grad *= gains;
 * update = momentum * update - learning_rate * grad; Y += update (fp32; gains start at 1 and the update at 0 in each
 * phase).  At iterations with (i + 1) % 50 == 0 the error and |grad| go to history and the phase stops when
 * i - best_iter > n_iter_without_progress (250 during exploration) without a new best error, or |grad| <=
 * min_grad_norm; a stop during exploration moves on to the second phase at i + 1, a stop in the second phase ends the
 * run.  The call enqueues max_iter iterations (one force and one step launch each); the iteration state lives in the
 * workspace, and after the run has ended every remaining launch returns at its entry.  history receives
 * [max_iter / 50 + 1][2] doubles (error, |grad|), DAD_TS_N_CHECKS of them written; out as above.
 * DAD_E_ARG: a NULL pointer, max_iter < 1, n_iter_without_progress < 0, early_exaggeration or learning_rate <= 0. */
typedef struct dad_tsne_args {
  int32_t max_iter;                  /* scikit-learn: 1000 */
  int32_t n_iter_without_progress;   /* 300 */
  double early_exaggeration;         /* 12 */
  double learning_rate;              /* 'auto' = max(n / early_exaggeration / 4, 50) */
  double min_grad_norm;              /* 1e-7 */
} dad_tsne_args;
int dad_tsne_run(const float* P, int64_t n, float* Y, const dad_tsne_args* args, double* history, double* out,
                 void* workspace, void* stream);

/* --- the clean-noisy domain gap of two splits' embeddings (csrc/domain_gap.hip) -----------
 * ECDALoss (I/utils.py:510-652) on whole splits instead of one batch.  emb [n][256] holds the rows of both domains
 * (dad_eval_split's emb of two splits, concatenated in any order), labels [n] their classes, domain [n] 0 for a
 * source / clean row and non-zero for a target / noisy one, weights [n] the rows' sample weights (NULL: all ones).
 * A row with a label outside [0, 4) takes no part in anything (how a caller applies a DACP mask); it and the rows
 * past n are left out by selection, so their values, NaN included, reach no sum.
 *
 * For a set S of m rows with D_ij = |x_i - x_j|^2:  bw = sum_ij D_ij / (m^2 - m) / 4 (0 for m < 2),
 * K_ij = sum_{b = 0 .. 4} exp(-D_ij / (bw 2^b + 1e-8))  (kernel_num = 5, kernel_mul = 2),
 * term_ss = sum_{i, j in src} w_i w_j K_ij / ((sum_src w)^2 + 1e-8), term_tt and term_st likewise (st: i in src, j in
 * tgt; the diagonal included), mmd = (ss + tt) - 2 st.
 * Per class c: S = the class's rows of both domains with their weights; gate_c = (n_src,c >= 2 and n_tgt,c >= 2), a
 * closed gate leaves zeros in the class's bandwidth, terms, mmd, compactness and shift; compactness_c = the mean of
 * |x - centroid_tgt,c|^2 over the class's target rows; shift_c = |centroid_src,c - centroid_tgt,c| (not in the
 * reference).  Global: S = every participating row with unit weights (the USE_CLASS_AWARE_MMD = False branch), gate
 * n_src >= 2 and n_tgt >= 2.  repulsion = -(mean pairwise distance of the target centroids of the classes with at
 * least one target row), 0 with fewer than two such classes.  attention_c = exp(lambda (mean(cw) - cw_c)).
 * ecda_loss = sum over open gates of attention_c (mmd_c + gamma compactness_c + delta repulsion): ECDALoss.forward.
 *
 * The distances are those of dad_cluster_metrics, squared (a Gram pass on the fp32 matrix cores on rows centred on
 * the participating rows' mean; duplicate rows are exactly 0 apart); the exponentials are v_exp_f32 on fp32
 * coefficients -log2(e) / (bw 2^b + 1e-8); row sums are fp32, everything across rows is double; centroids,
 * compactness, shift and repulsion are double arithmetic on the fp32 inputs.  Every sum has a fixed order (no
 * floating-point atomics): two calls on the same inputs write bit-identical outputs.  The calls only enqueue on
 * `stream` (no host synchronisation; graph-capturable).  out: DAD_DG_SLOTS doubles (device). */
#define DAD_DG_VALID 0            /* 1.0 when any gate, a class's or the global one, is open */
#define DAD_DG_N_SRC 1            /* participating source rows */
#define DAD_DG_N_TGT 2
#define DAD_DG_NONFINITE 3        /* participating rows with a non-finite component (the block is then meaningless) */
#define DAD_DG_REPULSION 4
#define DAD_DG_ECDA_LOSS 5
#define DAD_DG_MMD_CLASS_MEAN 6   /* mean mmd_c over the open gates (0 without one) */
#define DAD_DG_G_GATE 8           /* the global set */
#define DAD_DG_G_BANDWIDTH 9
#define DAD_DG_G_SS 10
#define DAD_DG_G_TT 11
#define DAD_DG_G_ST 12
#define DAD_DG_G_MMD 13
#define DAD_DG_C_GATE 16          /* [4] each from here on */
#define DAD_DG_C_BANDWIDTH 20
#define DAD_DG_C_SS 24
#define DAD_DG_C_TT 28
#define DAD_DG_C_ST 32
#define DAD_DG_C_MMD 36
#define DAD_DG_C_N_SRC 40
#define DAD_DG_C_N_TGT 44
#define DAD_DG_C_W_TGT 48         /* sum of the class's target weights */
#define DAD_DG_C_COMPACTNESS 52
#define DAD_DG_C_SHIFT 56
#define DAD_DG_C_ATTENTION 60
#define DAD_DG_SLOTS 64
#define DAD_DG_MAX_N 65536        /* largest n (both domains together) */
#define DAD_DG_TILE 64            /* rows / columns of a tile of the pairwise passes */
#define DAD_DG_MAX_CHUNKS 16      /* most column chunks a row tile is split into */
typedef struct dad_domain_gap_args {
  float class_weights[4];         /* cw (DACP's class weights; ones for the plain gap) */
  double lambda;                  /* ECDA_CLASS_ATTENTION_LAMBDA */
  double gamma;                   /* ECDA_COMPACTNESS_WEIGHT_GAMMA */
  double delta;                   /* ECDA_REPULSION_WEIGHT_DELTA */
} dad_domain_gap_args;
/* workspace bytes of dad_domain_gap (0 for an unsupported n); no initialisation needed */
size_t dad_domain_gap_workspace_bytes(int64_t n);
/* The grid of the two pairwise passes for n rows on a device of `cus` compute units, as dad_cluster_plan.  Host only. */
int dad_domain_gap_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk);
/* DAD_E_ARG: emb, labels, domain, args, out or workspace is NULL; DAD_E_SHAPE: n < 1 or n > DAD_DG_MAX_N. */
int dad_domain_gap(const float* emb, const int64_t* labels, const uint8_t* domain, const float* weights, int64_t n,
                   const dad_domain_gap_args* args, double* out, void* workspace, void* stream);
/* dad_domain_gap with the chunk count asked for (clamped as dad_domain_gap_plan clamps it; <= 0: the plan's), for
 * tests of the chunked summation at small n. */
int dad_domain_gap_chunked(const float* emb, const int64_t* labels, const uint8_t* domain, const float* weights,
                           int64_t n, const dad_domain_gap_args* args, double* out, int chunks, void* workspace,
                           void* stream);

/* --- exact k nearest neighbours of a split's embeddings and their scores (csrc/knn.hip) ----
 * Not in the reference; the yardstick is scikit-learn 1.7.2 (NearestNeighbors(algorithm='brute'),
 * KNeighborsClassifier(weights='uniform'), sklearn.manifold.trustworthiness).  Every call only enqueues on `stream`
 * (no host synchronisation; graph-capturable) and uses no floating-point atomics.  One workspace of
 * dad_knn_workspace_bytes(n, k) serves dad_knn and dad_trustworthiness; it needs no initialisation.
 *
 * dad_knn: the k nearest candidates of every row of emb [n][256] (dad_eval_split's emb / t_emb).  group [n] (NULL:
 * every row in group 0): a row with group < 0 is neither a query nor a candidate, and is left out by selection (its
 * values, NaN included, reach no other row's result).  The candidates of row i are the participating rows j != i
 * with, by mode, DAD_KNN_ALL: every one; DAD_KNN_SAME: group[j] == group[i]; DAD_KNN_OTHER: group[j] != group[i]
 * (group = the domain: one call answers noisy -> clean and clean -> noisy).  The distance is D_ij = max(|a_i|^2 +
 * |a_j|^2 - 2 a_i.a_j, 0) on the fp32 matrix cores, a = the rows minus the fp32 mean of the participating rows, |a_i|^2
 * the diagonal of the same Gram block -- with group NULL the bits dad_tsne_affinities sees, and dad_cluster_metrics'
 * distances squared.  The order is ascending in the pair (D_ij, j): ties go to the smaller index, a stable argsort.
 * idx [n][k] int32 and d2 [n][k] floats (device) receive the neighbours and their D; entries a row has no candidate
 * for (fewer than k candidates, or a row that takes no part) are -1 and +inf.  The selection is a total order on
 * bits that do not depend on the chunking: every chunk count, and every call, writes the same bits.  Rows past n are
 * never read.  The participating rows with a non-finite component are counted into the int32 at word
 * DAD_KNN_WS_NONFINITE of the workspace (idx and d2 are then meaningless).
 * DAD_E_ARG: emb, idx, d2 or workspace is NULL, or an unknown mode; DAD_E_SHAPE: k outside [1, DAD_KNN_MAX_K] or n
 * outside [1, DAD_KNN_MAX_N]. */
#define DAD_KNN_ALL 0
#define DAD_KNN_SAME 1
#define DAD_KNN_OTHER 2
#define DAD_KNN_MAX_K 32
#define DAD_KNN_MAX_N 65536
#define DAD_KNN_TILE 64           /* rows / columns of a tile of the pairwise pass */
#define DAD_KNN_MAX_CHUNKS 16     /* most column chunks a row tile is split into */
#define DAD_KNN_WS_NONFINITE 0    /* int32 word of the workspace: participating rows with a non-finite component */
/* workspace bytes of dad_knn / dad_trustworthiness (0 for an unsupported n or k) */
size_t dad_knn_workspace_bytes(int64_t n, int k);
int dad_knn(const float* emb, const int32_t* group, int64_t n, int k, int mode, int32_t* idx, float* d2,
            void* workspace, void* stream);
/* The grid of the pairwise pass for n rows and k neighbours on a device of `cus` compute units, as
 * dad_cluster_plan (up to k = 16 two workgroups share a compute unit, above it one: the lists live in LDS).
 * Host only. */
int dad_knn_plan(int64_t n, int k, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk);
/* dad_knn with the chunk count asked for (clamped as dad_knn_plan clamps it; <= 0: the plan's), for tests. */
int dad_knn_chunked(const float* emb, const int32_t* group, int64_t n, int k, int mode, int32_t* idx, float* d2,
                    int chunks, void* workspace, void* stream);
/* dad_knn_vote: the uniform vote over idx [n][k] (dad_knn's).  Each neighbour j >= 0 with labels[j] in [0, 4) casts
 * one vote; the first maximum wins (the smallest class on a tie, scikit-learn's rule).  pred [n] int64: the winner,
 * -1 for a row without a voting neighbour or with group < 0 (group NULL: every row in group 0).  out
 * [DAD_KV_SLOTS] int64 (device; the call clears it): over the query rows -- group >= 0 and an own label in [0, 4) --
 * confusion[g][label][pred] with g = (group != 0), the query count per g, and per g the queries without a vote (in
 * no confusion cell).  DAD_E_ARG: idx, labels, pred or out is NULL; DAD_E_SHAPE: as dad_knn. */
#define DAD_KV_CONFUSION 0        /* [2][4][4] */
#define DAD_KV_QUERIES 32         /* [2] */
#define DAD_KV_NO_VOTE 34         /* [2] */
#define DAD_KV_SLOTS 40
int dad_knn_vote(const int32_t* idx, const int64_t* labels, const int32_t* group, int64_t n, int k, int64_t* pred,
                 int64_t* out, void* stream);
/* dad_trustworthiness: sklearn.manifold.trustworthiness(emb, Y, n_neighbors = k) for Y [n][2] floats.  The k nearest
 * rows of each row in Y by (|y_i - y_j|^2, j), the distance (dx * dx) + (dy * dy) of the fp32 differences, each
 * operation rounded; for each such neighbour j the rank r(i, j) = 1 + #{l not in {i, j} : (D_il, l) < (D_ij, j)}
 * with dad_knn's D over all rows (scikit-learn leaves the order of equal distances to its sort; here it is the
 * index); penalty_i = sum_j max(0, r(i, j) - k); T = 1 - 2 sum_i penalty_i / (n k (2 n - 3 k - 1)) in double.  The
 * counts are int32 and exact, so the result does not depend on the chunking.  out [DAD_TW_SLOTS] doubles (device);
 * penalty [n] int32 (device, may be NULL) receives penalty_i.  DAD_E_ARG: emb, Y, out or workspace is NULL;
 * DAD_E_SHAPE: unless 1 <= k < n / 2 (scikit-learn's rule), k <= DAD_KNN_MAX_K and n <= DAD_KNN_MAX_N. */
#define DAD_TW_T 0
#define DAD_TW_PENALTY 1          /* sum_i penalty_i (exact below 2^53) */
#define DAD_TW_N 2
#define DAD_TW_K 3
#define DAD_TW_VALID 4            /* 1.0 when no row is non-finite */
#define DAD_TW_NONFINITE 5        /* rows of emb plus rows of Y with a non-finite component (T is then meaningless) */
#define DAD_TW_SLOTS 8
int dad_trustworthiness(const float* emb, const float* Y, int64_t n, int k, double* out, int32_t* penalty,
                        void* workspace, void* stream);
/* dad_trustworthiness with the chunk count of the counting pass asked for (<= 0: dad_knn_plan's), for tests. */
int dad_trustworthiness_chunked(const float* emb, const float* Y, int64_t n, int k, double* out, int32_t* penalty,
                                int chunks, void* workspace, void* stream);

/* --- the supervised-contrastive loss and its gradient (csrc/scl.hip) ----------------------
 * The reference names the term (SupervisedContrastiveLoss(temperature=0.1), TARGET_SCL_WEIGHT, SCL_START_EPOCH; "SCL -
 * class alignment", C/model.py:74) but deleted its code and hard-wires 0 (C/train_CASIA.py:396,442), so this text is
 * the definition: SupCon (Khosla et al. 2020, the "L_out" form) without a base-temperature factor.
 *
 * emb [n][256], labels [n], member [n] (a flag per row), tau > 0.  The member set A holds the flagged rows with a
 * label in [0, 4) and |e_i| > 1e-12 (a row without a direction is left out: the normalisation's backward would
 * otherwise be of order 1e12).  Rows outside A are left out by selection: their values, NaN included, reach no sum,
 * and their gradient is 0.  With z_i = e_i / |e_i|, s_ia = z_i . z_a and P(i) = {p in A, p != i, y_p = y_i}:
 *   l_i = -(1 / |P(i)|) sum_{p in P(i)} [ s_ip / tau - log sum_{a in A, a != i} exp(s_ia / tau) ]
 *   L   = mean of l_i over the V anchors with |P(i)| >= 1;  L = 0 with a zero gradient when V = 0.
 * Gradient, in closed form: p_ia = softmax over a != i of s_ia / tau, v_i = [|P(i)| >= 1], c_i = v_i / |P(i)|,
 *   H_ia = (v_i p_ia - c_i [a in P(i)]) / (V tau),  G = H + H^T,  gz_i = sum_a G_ia z_a,
 *   dL/de_i = (gz_i - z_i (z_i . gz_i)) / |e_i|.
 * Two n x n passes over the Gram block of the unit rows on the fp32 matrix cores: the first takes each row's
 * log-sum-exp under a running row maximum (no tau > 0 overflows or meets log 0) and its positives' sum, the second
 * forms G tile by tile and accumulates G Z with MFMA; an epilogue applies the normalisation's backward.  The norms and
 * the loss are reduced in double, the rest is fp32.  Enqueue-only on `stream` (graph-capturable), no floating-point
 * atomics, every sum in a fixed order (two calls write bit-identical outputs), no counter or spin-wait between
 * workgroups: the stream alone orders the four launches.  Rows past n are never read.
 * out [DAD_SCL_SLOTS] floats (device); grad [n][256] (device, may be NULL: then only out is written).
 * DAD_E_ARG: emb, labels, member, out or workspace is NULL, or tau is <= 0 or not finite (before anything is
 * launched); DAD_E_SHAPE: n < 1 or n > DAD_SCL_MAX_N. */
#define DAD_SCL_LOSS 0
#define DAD_SCL_V 1               /* anchors: members whose class has another member */
#define DAD_SCL_MEMBERS 2         /* |A| */
#define DAD_SCL_ANCHORS 3         /* [4] anchors per class */
#define DAD_SCL_NONFINITE 7       /* flagged rows (label in range) with a non-finite component (the block is then
                                     meaningless) */
#define DAD_SCL_SLOTS 8
#define DAD_SCL_MAX_N 2048        /* largest n: 2 * DAD_MAX_BATCH, the step's largest batch */
#define DAD_SCL_TILE 64           /* rows / columns of a tile of the pairwise passes */
#define DAD_SCL_MAX_CHUNKS 8      /* most column chunks a row tile is split into */
/* workspace bytes of dad_scl (0 for an unsupported n); no initialisation needed */
size_t dad_scl_workspace_bytes(int64_t n);
/* The grid of the two pairwise passes for n rows on a device of `cus` compute units, as dad_cluster_plan (one
 * workgroup per compute unit).  Host only. */
int dad_scl_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk);
int dad_scl(const float* emb, const int64_t* labels, const uint8_t* member, int64_t n, float tau, float* out,
            float* grad, void* workspace, void* stream);
/* dad_scl with the chunk count asked for (clamped as dad_scl_plan clamps it; <= 0: the plan's), for tests of the
 * chunked combination at small n. */
int dad_scl_chunked(const float* emb, const int64_t* labels, const uint8_t* member, int64_t n, float tau, float* out,
                    float* grad, int chunks, void* workspace, void* stream);

/* --- rank a split by a key and count positives along the order (csrc/rank.hip) -------------
 * DACP keeps a pseudo-label when the teacher's certainty score clears a per-class quantile threshold
 * (I/utils.py:449-507).  Whether that score is any good -- the coverage and purity a threshold buys, the split-wide
 * quantiles, the wrong labels that pass, ROC-AUC, average precision, the risk-coverage curve, the reference's
 * confidence_stats (I/inference.py:361-369) -- is one computation: put rows in a total order by a key and count
 * positives along it.  m columns of n rows each, all inputs on the device and never written:
 *   key [m][n] float32; flags [m][n] uint8 (DAD_RK_MEMBER | DAD_RK_POSITIVE); thr [m] float32 (NaN: no threshold);
 *   gammas [Q] float32; B bins over [bin_lo, bin_hi), shared by the columns.
 * Row i takes part in column j when its member bit is set and key[j][i] is finite (M rows; a member with a
 * non-finite key is counted in DAD_RK_NONFINITE and left out).  The order of a column is over its M rows by
 * (key descending, row index ascending); keys compare as values, so -0.0 equals +0.0 (and is reported as +0.0).
 * Outputs per column (order, cum_pos, tie_end may each be NULL):
 *   order [m][n] int32     the rows in order at positions 0 .. M-1, -1 behind them
 *   cum_pos [m][n] int32   positives among positions 0 .. k; 0 at positions >= M
 *   tie_end [m][n] uint8   1 where position k ends a run of equal keys: a curve is defined at these points only,
 *                          which makes it independent of the order of the rows
 *   counts [m][DAD_RK_COUNTS] int64, values [m][DAD_RK_VALUES] double: the slots below; an undefined value is 0
 *   quant [m][Q] float32   torch.quantile(keys, gamma) (linear) of the M keys, in the float32 arithmetic of the
 *                          step's DACP threshold: rank gamma (M - 1), lerp with the w < 0.5 branch; NaN for M = 0
 *   bin_counts [m][B][2] int64 (rows, positives) and bin_sum [m][B] double (sum of the keys); the bin of a key is
 *                          floor((double(key) - lo) / (hi - lo) * B) clamped to [0, B - 1]
 * Every integer is exact.  Every double is a sum over the positions of the order in one fixed order that depends on
 * nothing but the sorted sequence (no floating-point atomics): two calls, every chunk count and every permutation of
 * the rows write the same bits to counts, values, quant and the bin blocks.  Enqueue-only on `stream`. */
#define DAD_RK_MEMBERS 0          /* M: rows that take part */
#define DAD_RK_POSITIVES 1        /* P: positives among them */
#define DAD_RK_NONFINITE 2        /* members with a non-finite key (left out) */
#define DAD_RK_RUNS 3             /* runs of equal keys */
#define DAD_RK_U2 4               /* 2 #{key_p > key_q} + #{key_p = key_q} over (positive p, negative q): the
                                     Mann-Whitney count, roc_auc_score = U2 / (2 P (M - P)) exactly */
#define DAD_RK_ACCEPTED 5         /* rows with key >= thr (I/utils.py:501); 0 for a NaN thr */
#define DAD_RK_ACCEPTED_POS 6     /* positives among them */
#define DAD_RK_VALID_AUROC 7      /* 0 when P = 0 or P = M */
#define DAD_RK_COUNTS 8
#define DAD_RK_AUROC 0
#define DAD_RK_AP 1               /* scikit-learn's average_precision_score: sum over runs of (R_r - R_{r-1}) P_r */
#define DAD_RK_AURC 2             /* (1 / M) sum over runs of size_r (accepted_r - cum_pos_r) / accepted_r */
#define DAD_RK_KEY_MEAN 3         /* the reference's confidence_stats: mean, population std, min, max */
#define DAD_RK_KEY_STD 4
#define DAD_RK_KEY_MIN 5
#define DAD_RK_KEY_MAX 6
#define DAD_RK_VALUES 8
#define DAD_RK_MEMBER 1           /* flag bits */
#define DAD_RK_POSITIVE 2
#define DAD_RK_MAX_N 65536        /* largest n, as DAD_CM_MAX_N */
#define DAD_RK_MAX_M 16           /* most columns */
#define DAD_RK_MAX_Q 8            /* most quantiles */
#define DAD_RK_MAX_BINS 64        /* most bins */
#define DAD_RK_TILE 256           /* rows of a row tile / keys of a key tile of the counting pass */
#define DAD_RK_MAX_CHUNKS 8       /* most chunks the key tiles of a row tile are split into */
#define DAD_RK_EVAL_COLUMNS 10    /* columns dad_rank_eval_columns writes */
typedef struct dad_rank_args {
  const float* key;
  const uint8_t* flags;
  const float* thr;
  const float* gammas;            /* may be NULL when Q = 0 */
  int32_t* order;                 /* may be NULL */
  int32_t* cum_pos;               /* may be NULL */
  uint8_t* tie_end;               /* may be NULL */
  int64_t* counts;
  double* values;
  float* quant;                   /* may be NULL when Q = 0 */
  int64_t* bin_counts;            /* may be NULL when B = 0 */
  double* bin_sum;                /* may be NULL when B = 0 */
  int64_t n;
  int32_t m, Q, B;
  float bin_lo, bin_hi;
  int32_t reserved;
} dad_rank_args;
/* workspace bytes of dad_rank_metrics (0 for an unsupported n or m); no initialisation needed */
size_t dad_rank_workspace_bytes(int64_t n, int m);
/* The grid of the counting pass for n rows and m columns on a device of `cus` compute units: workgroup
 * (row tile, chunk, column), the key tiles of a column in `chunks` contiguous runs of `tiles_per_chunk` (no chunk
 * empty), chunks <= min(row tiles, DAD_RK_MAX_CHUNKS).  Host only. */
int dad_rank_plan(int64_t n, int m, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk);
/* DAD_E_ARG: args, workspace or a required pointer is NULL, or with B > 0 a range that is not finite with
 * bin_lo < bin_hi; DAD_E_SHAPE: n outside [1, DAD_RK_MAX_N], m outside [1, DAD_RK_MAX_M], Q outside
 * [0, DAD_RK_MAX_Q] or B outside [0, DAD_RK_MAX_BINS].  Nothing is launched on an error. */
int dad_rank_metrics(const dad_rank_args* args, void* workspace, void* stream);
/* dad_rank_metrics with the chunk count asked for (clamped as dad_rank_plan clamps it; <= 0: the plan's), for
 * tests of the chunked counts at small n. */
int dad_rank_metrics_chunked(const dad_rank_args* args, int chunks, void* workspace, void* stream);
/* The ten standard columns of an evaluated split, key [10][n] and flags [10][n], from dad_eval_split's score [n],
 * probs [n][4], pred [n] and labels [n] (one small kernel):
 *   0     key = score, positive = the prediction is correct (selective classification)
 *   1-4   key = score, member = pred is c, positive = label is c: DACP's per-class gate, precision is purity
 *   5     key = max probability, positive = correct
 *   6-9   key = p_c, positive = label is c (one-vs-rest)
 * A row whose label or prediction is outside [0, 4) is a member of nothing.  labels NULL: every row (with a
 * prediction in range) is a member and none is positive, so quantiles and gate counts still work on an unlabelled
 * split.  DAD_E_ARG: score, probs, pred, key or flags is NULL; DAD_E_SHAPE: n outside [1, DAD_RK_MAX_N]. */
int dad_rank_eval_columns(const float* score, const float* probs, const int64_t* pred, const int64_t* labels,
                          int64_t n, float* key, uint8_t* flags, void* stream);

/* --- the reference's helper types as operators (I/utils.py:317-652) -------------------
 * For trainer code that drives DataAugmentation / DACPManager / ECDALoss itself (the
 * train_step shim's callers, anchor calibration, I/train.py:334,341).  Same device functions
 * as the fused step.
 *
 * DataAugmentation.weak_augment (strong = 0, I/utils.py:328-331) / strong_augment (strong = 1,
 * I/utils.py:333-375) of x [B][T][D] (a [T][D] input is B = 1; 1-D or > 3-D inputs are
 * passed with mask_len 0, as the reference masks only 2-D / 3-D data):
 *   out = x + std * N;  strong: * (u[d] > feat_p) (one [D] mask, no rescale; skipped when
 *   feat_p <= 0), then frames [start_b, start_b + mask_len) of utterance b zeroed, start_b
 *   uniform in [0, max(1, T - mask_len + 1)).
 * Draws: explicit (noise [B][T][D] standard normals, u [D] uniforms, start [B]) or, for NULL,
 * the counter streams of (seed, counter) -- with D = 768 the values the fused step draws. */
int dad_augment(const float* x, int B, int T, int D, int strong, float noise_std, float feat_p, int mask_len,
                uint64_t seed, uint64_t counter, const float* noise, const float* u, const int64_t* start,
                float* out, void* stream);
/* DACPManager.calculate_certainty_scores (I/utils.py:400-428): probs [B][4] -> score [B],
 * pred [B] (first argmax); use_entropy = USE_ENTROPY_IN_SCORE.  Outputs may be NULL. */
int dad_certainty_scores(const float* probs, int B, int use_entropy, float* score, int64_t* pred, void* stream);
/* DACPManager.calculate_mask (I/utils.py:449-507): teacher probs [Bn][4] and the 20-float
 * DACP state (tau | Q | epoch score sums | counts | calibrated anchors, DAD_DACP_FLOATS) ->
 * mask [Bn] (1 = confident), score [Bn], pred [Bn], class_weights [4] (W_c); updates tau
 * (EMA of the floored thresholds) and the epoch sums / counts in place, as the reference
 * updates its fields.  Reads cfg: dacp_gamma (from the epoch), dacp_k, dacp_lambda,
 * dacp_alpha / one_m_alpha, use_entropy.  score / pred / class_weights may be NULL. */
int dad_dacp_mask(const dad_config* cfg, const float* probs, int Bn, float* dacp, uint8_t* mask, float* score,
                  int64_t* pred, float* class_weights, void* stream);
/* ECDALoss.forward (I/utils.py:565-652) + its gradients: clean [B][256], noisy [Bn][256]
 * embeddings, clean_labels [B], noisy_labels [Bn] (teacher pseudo-labels), noisy_mask [Bn]
 * (1 = confident), noisy_scores [Bn], class_weights [n_weights] (DACP's [4] W_c, or the
 * fixed-threshold branch's ones(Bn), I/train.py:420).  loss [1] (device) = the class-aware sum
 * (or the global-MMD ablation when cfg->class_aware = 0); grad_clean [B][256] / grad_noisy
 * [Bn][256] = d loss / d embeddings (rows outside every member set are 0; may be NULL).
 * Reads cfg: class_aware, ecda_att_lambda, ecda_gamma, ecda_delta.
 * workspace: dad_ecda_workspace_bytes(B, Bn). */
size_t dad_ecda_workspace_bytes(int B, int Bn);
int dad_ecda_loss(const dad_config* cfg, const float* clean, int B, const float* noisy, int Bn,
                  const int64_t* clean_labels, const int64_t* noisy_labels, const uint8_t* noisy_mask,
                  const float* noisy_scores, const float* class_weights, int n_weights, float* loss,
                  float* grad_clean, float* grad_noisy, void* workspace, void* stream);

/* --- counter-RNG draws (diagnostics, distribution tests) ------------------------------
 * The random draws the throughput mode (DAD_RNG_COUNTER) makes inside the step kernels for
 * the step described by cfg (seed, counter = global step, B / Bn / Tn, stds, p, mask
 * geometry), computed by the same device functions the kernels call.  Elements
 * [first, first + n) of one stream, as float:
 *   DAD_DRAW_WEAK       weak-aug noise std*N of element i of the [Bn][Tn][768] tensor
 *                       (DataAugmentation.weak_augment's randn_like * std, I/utils.py:330)
 *   DAD_DRAW_STRONG     strong-aug noise (I/utils.py:338)
 *   DAD_DRAW_FEAT_KEEP  feature keep flag 1/0 of channel d < 768 (rand(D) > p, I/utils.py:343)
 *   DAD_DRAW_TSTART     temporal-mask start of utterance b < Bn (randint, I/utils.py:370)
 *   DAD_DRAW_KEEP1      classifier dropout factor (0 or 1/(1-p)) of element b*256+h, b < B
 *                       (student_classifier dropout, clean pass, I/train.py:400)
 *   DAD_DRAW_KEEP2      same, strong pass, b < Bn (I/train.py:440) */
#define DAD_DRAW_WEAK 1
#define DAD_DRAW_STRONG 2
#define DAD_DRAW_FEAT_KEEP 3
#define DAD_DRAW_TSTART 4
#define DAD_DRAW_KEEP1 5
#define DAD_DRAW_KEEP2 6
int dad_rng_draws(const dad_config* cfg, int which, uint64_t first, size_t n, float* out, void* stream);

/* --- per-kernel timing of the fused step (diagnostics; not inside graph capture) ------
 * dad_timing_start(every, max_steps): from now on every `every`-th step (counted at its
 * dad_step_encode / dad_step_compute call) records hip events at the boundaries of its kernels
 * on the caller's stream, up to max_steps timed steps; all events are created here, so a timed
 * region only records them.  dad_timing_stop: waits for the recorded events and returns, per
 * kernel k < n (DAD_TK_*), the summed milliseconds ms_sum[k] over count[k] timed steps, then
 * frees the events and turns timing off.  dad_timing_start fails (DAD_E_ARG) while a timing
 * session is active: stop the first before starting another. */
#define DAD_TK_ENCODE 0       /* dad_encode_ws[_f16] / dad_encode_f32 */
#define DAD_TK_POOL 1         /* dad_pool */
#define DAD_TK_TAIL 2         /* dad_tail_ecda_w / dad_tail_ecda (warm-up: dad_tail); with dad_config.scl_on also
                                 dad_scl's four launches behind it */
#define DAD_TK_WGRAD 3        /* dad_wgrad_direct (FP16/BF16) / dad_wgrad_f32 (FP32) */
#define DAD_TK_REDUCE 4       /* dad_reduce_w (FP16/BF16) / dad_reduce (FP32) */
#define DAD_TK_OPTIM 5        /* dad_optim */
#define DAD_TK_KERNELS 6
int dad_timing_start(int every, int max_steps);
/* dad_timing_kernels(mask): after dad_timing_start, record only the boundaries of the kernels
 * whose bit (1 << DAD_TK_*) is set (default: all).  Each recorded event costs the stream a few
 * microseconds, so a timed region that needs one kernel's duration records only its two. */
int dad_timing_kernels(unsigned mask);
/* dad_timing_reset (ABI 7): forget the steps counted and recorded so far in the active session (its
 * events stay created); the next step is the session's step 0.  A timed region can then follow its
 * warm-up with no gap: dad_timing_start's event set-up (milliseconds of host time with the GPU idle)
 * runs before the warm-up, the reset between them. */
int dad_timing_reset(void);
int dad_timing_stop(double* ms_sum, int* count, int n);

/* --- data-parallel gradient exchange (RCCL over xGMI) ------------------------------ */
int dad_comm_unique_id_bytes(void);
int dad_comm_get_unique_id(void* id_out);
int dad_comm_init(void** comm, int nranks, const void* id, int rank);
/* in-place SUM all-reduce of state->grad (DAD_GRAD_FLOATS floats) on `stream` */
int dad_comm_allreduce_grad(void* comm, const dad_state* st, void* stream);
/* ranks in the communicator (ncclCommCount) */
int dad_comm_count(void* comm, int* nranks);
/* in-place SUM all-reduce of n floats on `stream` (bench/test probe: a buffer of ones
 * all-reduced gives the number of ranks the transport actually connected) */
int dad_comm_allreduce_f32(void* comm, float* buf, size_t n, void* stream);
int dad_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* DAD_ABI_H_ */
