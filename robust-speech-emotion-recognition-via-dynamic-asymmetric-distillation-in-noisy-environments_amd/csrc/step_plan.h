// The host plan of one DAD step: which entry point each of its launches is (the `_s16` / `_rg` siblings
// included) and how large its grid, decided in one place (plan_step) from the configs and the batch
// structs' own fields (which pointers are present, the store row types).  Host code only: no HIP call,
// no allocation, nothing read through a batch pointer.  The step's enqueue code (dad_abi.hip) launches
// what the plan says; dad_step_plan and dad_step_plan_kernels (dad.h) show the same plan to tests.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dad_kernels.h"
#include "scl.h"

inline int check_cfg(const dad_config* c) {
  if (!c) return DAD_E_ARG;
  if (c->B < 1 || c->B > DAD_MAX_BATCH || c->T < 1) return DAD_E_SHAPE;
  if (c->Bn < 0 || c->Bn > DAD_MAX_BATCH || c->Tn < 0) return DAD_E_SHAPE;
  if (!c->warmup && (c->Bn < 1 || c->Tn < 1)) return DAD_E_SHAPE;
  if (c->precision != DAD_PREC_FP32 && !dad_prec16(c->precision)) return DAD_E_ARG;
  if (c->rng_mode != DAD_RNG_EXPLICIT && c->rng_mode != DAD_RNG_COUNTER) return DAD_E_ARG;
  if (c->dp_world < 1) return DAD_E_ARG;
  if (c->ragged && !dad_prec16(c->precision)) return DAD_E_UNSUPPORTED;   // (ragged mode: the 16-bit store-fed steps)
  if (c->scl_on && !(scl_tau_ok(c->scl_tau) && c->w_scl >= -3.402823466e38f && c->w_scl <= 3.402823466e38f)) return DAD_E_ARG;
  return DAD_OK;
}

// the step runs the supervised-contrastive term: switched on, and past the warm-up (which is CE only)
inline bool scl_in_step(const dad_config* c) { return c->scl_on && !c->warmup; }

inline DadGeom geom_of(const dad_config* c) { return dad_geom(c->B, c->T, c->Bn, c->Tn); }

// Batch-pointer checks shared by the step, can_prepare_ahead and dad_step_prepare_rows.
// Store mode, per batch (clean and noisy independently): rows and lengths come together.
inline bool rows_paired(const dad_batch* b) {
  return (b->rowc == nullptr) == (b->lenc == nullptr) && (b->rown == nullptr) == (b->lenn == nullptr);
}
// The element types of a batch's feature rows (dad_batch.xc_dtype / xn_dtype): a padded batch is
// f32; a 16-bit store is read in place by the 16-bit steps' row preparation only (the exact-f32
// encoder and weight gradient read f32 rows).
inline bool store_dtype_ok(int t) { return t == DAD_STORE_F32 || t == DAD_STORE_F16 || t == DAD_STORE_BF16; }
inline int check_batch_dtypes(const dad_config* c, const dad_batch* b) {
  if (!store_dtype_ok(b->xc_dtype) || !store_dtype_ok(b->xn_dtype)) return DAD_E_ARG;
  if ((!b->rowc && b->xc_dtype != DAD_STORE_F32) || (!b->rown && b->xn_dtype != DAD_STORE_F32)) return DAD_E_ARG;
  if ((b->xc_dtype != DAD_STORE_F32 || b->xn_dtype != DAD_STORE_F32) && !dad_prec16(c->precision))
    return DAD_E_UNSUPPORTED;
  return DAD_OK;
}
// Ragged mode reads the lengths of every batch side that is present: both must be store batches.
inline int check_ragged_batch(const dad_config* c, const dad_batch* b) {
  if (!c->ragged) return DAD_OK;
  if (!b->rowc || !b->lenc) return DAD_E_ARG;
  if ((b->xn || !c->warmup) && (!b->rown || !b->lenn)) return DAD_E_ARG;
  return DAD_OK;
}
// DAD_RNG_EXPLICIT: the augmentation's four draws of a noisy batch
inline bool has_explicit_draws(const dad_batch* b) { return b->nw && b->ns && b->u && b->start; }

inline int splits_of(const dad_config* c) {
  const DadGeom g = geom_of(c);
  if (c->splits <= 0) return dad_auto_splits(g, c->precision, c->warmup);
  if (!dad_prec16(c->precision)) return c->splits;
  // dad_wgrad_direct holds at most WGD_MAXU slabs' utterances per split
  return std::max(c->splits, dad_wgd_min_splits(dad_wg_total(g, c->warmup)));
}

inline int max_splits_of(const dad_config* c) {
  // the workspace is sized for the largest split count any step with this geometry may use
  const int s = splits_of(c);
  if (!c->warmup) return s;
  dad_config post = *c;
  post.warmup = 0;
  return std::max(s, splits_of(&post));
}

// DAD_TAIL_W=0 selects the general tail + ECDA launch for every batch (A/B runs; read once)
inline bool tail_w_on() {
  static const bool on = [] { const char* e = getenv("DAD_TAIL_W"); return !(e && strcmp(e, "0") == 0); }();
  return on;
}

// Roles of the prepared-row encoder (dad_encode_wp, dad_wp_job_range): nt teacher and ns student
// workgroups, one per CU, in proportion to their live 16-row sub-slabs (every prepared sub-slab
// costs the same); more workgroups than CUs only when a range would exceed the kernel's
// DAD_ENC_WS_MAXJ-job table.
inline int wp_max_range(const DadGeom& G, int Bn, int nt, int ns) {
  int worst = 0;
  for (int wg = 0; wg < nt + ns; ++wg) {
    bool t = false;
    int j0 = 0, j1 = 0;
    dad_wp_job_range(wg, nt, ns, G.Bc, G.Tc, G.ncc, Bn, G.Tn, G.ncn, Bn * G.ncn, t, j0, j1);
    worst = std::max(worst, j1 - j0);
  }
  return worst;
}
inline int wp_split(const DadGeom& G, int Bn, int cus, int& nt, int& ns) {
  struct Entry { int Bc, Tc, Bn, Tn, cus, rc, nt, ns; };
  static thread_local Entry last{-1, -1, -1, -1, -1, 0, 0, 0};
  if (!(last.Bc == G.Bc && last.Tc == G.Tc && last.Bn == Bn && last.Tn == G.Tn && last.cus == cus)) {
    Entry e{G.Bc, G.Tc, Bn, G.Tn, cus, 0, 0, 0};
    const int Js = Bn * G.ncn, Jc = G.Bc * G.ncc;
    const double ln = (double)Bn * ((G.Tn + 15) / 16), lc = (double)G.Bc * ((G.Tc + 15) / 16);
    if (Js == 0) {
      e.ns = std::min(cus, Jc);
    } else {
      e.nt = std::max(1, std::min(std::min(Js, cus - 1), (int)(cus * ln / (2.0 * ln + lc) + 0.5)));
      e.ns = std::min(cus - e.nt, Jc + Js);
    }
    while (e.rc == DAD_OK && wp_max_range(G, Bn, e.nt, e.ns) > DAD_ENC_WS_MAXJ) {
      if (e.nt > 0 && e.nt < Js) ++e.nt;
      if (e.ns < Jc + Js) ++e.ns;
      if (e.nt + e.ns > Js + Jc + 2) e.rc = DAD_E_SHAPE;
    }
    last = e;
  }
  nt = last.nt;
  ns = last.ns;
  return last.rc;
}

// standalone dad_prep: ~4 workgroups of 4 waves per CU, two rows in flight per wave
inline int prep_grid_of(int cus) { return 4 * cus; }

// Every entry point a step can launch, once: X(id, entry point, family, argument blocks, block size).  The
// StepKernel enum and kStepKernels below and the launch table (dad_host.h) are all expansions of this
// list, so none of them can fall out of step with another.  The name is the entry point's, spelt as the
// profile tools do.  The family is the kernel dad_step_plan_info reports for it: a base kernel its own,
// an `_s16` / `_rg` sibling (dad_kernels.h) the kernel it stands in for.  The argument blocks (KernelSig)
// say which launch helper takes it.
#define DAD_STEP_KERNELS(X)                                                                              \
  X(K_PREP, dad_prep, K_PREP, SIG_PREP, DAD_PREP_THREADS)                                                \
  X(K_PREP_S16, dad_prep_s16, K_PREP, SIG_PREP, DAD_PREP_THREADS)                                        \
  X(K_PREP_RG, dad_prep_rg, K_PREP, SIG_PREP, DAD_PREP_THREADS)                                          \
  X(K_ENCODE_F32, dad_encode_f32, K_ENCODE_F32, SIG_ENCODE, DAD_ENC_F32_THREADS)                         \
  X(K_ENCODE_WP, dad_encode_wp, K_ENCODE_WP, SIG_ENCODE, DAD_ENC_WS_THREADS)                             \
  X(K_ENCODE_WP_F16, dad_encode_wp_f16, K_ENCODE_WP_F16, SIG_ENCODE, DAD_ENC_WS_THREADS)                 \
  X(K_ENCODE_WP_RG, dad_encode_wp_rg, K_ENCODE_WP, SIG_ENCODE, DAD_ENC_WS_THREADS)                       \
  X(K_ENCODE_WP_F16_RG, dad_encode_wp_f16_rg, K_ENCODE_WP_F16, SIG_ENCODE, DAD_ENC_WS_THREADS)           \
  X(K_POOL, dad_pool, K_POOL, SIG_POOL, DAD_POOL_THREADS)                                                \
  X(K_POOL_RG, dad_pool_rg, K_POOL, SIG_POOL, DAD_POOL_THREADS)                                          \
  X(K_TAIL, dad_tail, K_TAIL, SIG_TAIL, DAD_TAIL_THREADS)                                                \
  X(K_TAIL_ECDA, dad_tail_ecda, K_TAIL_ECDA, SIG_TAIL_ECDA, DAD_TAIL_THREADS)                            \
  X(K_TAIL_ECDA_W, dad_tail_ecda_w, K_TAIL_ECDA_W, SIG_TAIL_W, DAD_TAIL_THREADS)                         \
  X(K_TAIL_ECDA_W_S16, dad_tail_ecda_w_s16, K_TAIL_ECDA_W, SIG_TAIL_W, DAD_TAIL_THREADS)                 \
  X(K_TAIL_ECDA_W_RG, dad_tail_ecda_w_rg, K_TAIL_ECDA_W, SIG_TAIL_W, DAD_TAIL_THREADS)                   \
  X(K_WGRAD_F32, dad_wgrad_f32, K_WGRAD_F32, SIG_WGRAD, DAD_WGRAD_THREADS)                               \
  X(K_WGRAD_DIRECT, dad_wgrad_direct, K_WGRAD_DIRECT, SIG_WGRAD, WGD_THREADS)                            \
  X(K_WGRAD_DIRECT_CP, dad_wgrad_direct_cp, K_WGRAD_DIRECT_CP, SIG_WGRAD_CP, WGD_THREADS)                \
  X(K_WGRAD_DIRECT_CPS, dad_wgrad_direct_cps, K_WGRAD_DIRECT_CPS, SIG_WGRAD_CP, WGD_THREADS)             \
  X(K_WGRAD_DIRECT_F16, dad_wgrad_direct_f16, K_WGRAD_DIRECT_F16, SIG_WGRAD, WGD_THREADS)                \
  X(K_WGRAD_DIRECT_F16_CP, dad_wgrad_direct_f16_cp, K_WGRAD_DIRECT_F16_CP, SIG_WGRAD_CP, WGD_THREADS)    \
  X(K_WGRAD_DIRECT_F16_CPS, dad_wgrad_direct_f16_cps, K_WGRAD_DIRECT_F16_CPS, SIG_WGRAD_CP, WGD_THREADS) \
  X(K_WGRAD_DIRECT_CPS_S16, dad_wgrad_direct_cps_s16, K_WGRAD_DIRECT_CPS, SIG_WGRAD_CP, WGD_THREADS)     \
  X(K_WGRAD_DIRECT_F16_CPS_S16, dad_wgrad_direct_f16_cps_s16, K_WGRAD_DIRECT_F16_CPS, SIG_WGRAD_CP, WGD_THREADS) \
  X(K_WGRAD_DIRECT_RG, dad_wgrad_direct_rg, K_WGRAD_DIRECT, SIG_WGRAD, WGD_THREADS)                      \
  X(K_WGRAD_DIRECT_F16_RG, dad_wgrad_direct_f16_rg, K_WGRAD_DIRECT_F16, SIG_WGRAD, WGD_THREADS)          \
  X(K_WGRAD_DIRECT_CPS_RG, dad_wgrad_direct_cps_rg, K_WGRAD_DIRECT_CPS, SIG_WGRAD_CP, WGD_THREADS)       \
  X(K_WGRAD_DIRECT_F16_CPS_RG, dad_wgrad_direct_f16_cps_rg, K_WGRAD_DIRECT_F16_CPS, SIG_WGRAD_CP, WGD_THREADS) \
  X(K_REDUCE, dad_reduce, K_REDUCE, SIG_REDUCE, DAD_REDUCE_THREADS)                                      \
  X(K_REDUCE_W, dad_reduce_w, K_REDUCE_W, SIG_REDUCE, 64)

#define DAD_X_ID(id, fn, family, sig, threads) id,
enum StepKernel { DAD_STEP_KERNELS(DAD_X_ID) K_COUNT };
#undef DAD_X_ID
// the argument blocks an entry point takes (dad_host.h SigOf spells each list out)
enum KernelSig { SIG_PREP, SIG_ENCODE, SIG_POOL, SIG_TAIL, SIG_TAIL_ECDA, SIG_TAIL_W, SIG_WGRAD, SIG_WGRAD_CP, SIG_REDUCE };
struct StepKernelInfo { const char* name; StepKernel family; KernelSig sig; int threads; };
#define DAD_X_INFO(id, fn, family, sig, threads) {#fn, family, sig, threads},
constexpr StepKernelInfo kStepKernels[K_COUNT] = {DAD_STEP_KERNELS(DAD_X_INFO)};
#undef DAD_X_INFO
inline const char* family_name(StepKernel k) { return kStepKernels[kStepKernels[k].family].name; }

// Kernel selection, shared by plan_step, dad_step_prepare_rows and the modular encoder ops.
// Rows that a launch prepares (DAD_PREP_* parts of (cfg, batch)'s set) lie in a 16-bit store, so the
// launch is the `_s16` form; batch NULL: a padded f32 batch.  Reads the struct's own fields only.
inline bool rows_need_s16(const dad_config* cfg, const dad_batch* batch, int parts) {
  if (!batch) return false;
  return ((parts & DAD_PREP_CLEAN) && batch->xc_dtype != DAD_STORE_F32) ||
         ((parts & DAD_PREP_NOISY) && !cfg->warmup && cfg->Bn > 0 && batch->xn_dtype != DAD_STORE_F32);
}
// the standalone preparation: the ragged sibling reads any store type, hence before the `_s16` one
inline StepKernel prep_kernel(bool ragged, bool s16) { return ragged ? K_PREP_RG : s16 ? K_PREP_S16 : K_PREP; }
inline StepKernel encode_kernel(int precision, bool ragged) {
  if (!dad_prec16(precision)) return K_ENCODE_F32;
  const bool f16 = precision == DAD_PREC_FP16;
  if (ragged) return f16 ? K_ENCODE_WP_F16_RG : K_ENCODE_WP_RG;
  return f16 ? K_ENCODE_WP_F16 : K_ENCODE_WP;
}
// the 16-bit weight gradient by [fp16][takes the next batch's clean rows][through its store table]
constexpr StepKernel kWgradDirect[2][2][2] = {
    {{K_WGRAD_DIRECT, K_WGRAD_DIRECT}, {K_WGRAD_DIRECT_CP, K_WGRAD_DIRECT_CPS}},
    {{K_WGRAD_DIRECT_F16, K_WGRAD_DIRECT_F16}, {K_WGRAD_DIRECT_F16_CP, K_WGRAD_DIRECT_F16_CPS}}};
// ... a ragged step's by [fp16][takes the (ragged, store) next batch's clean rows], and the `_cps`
// kernel's sibling for clean rows in a 16-bit store by [fp16]
constexpr StepKernel kWgradDirectRg[2][2] = {{K_WGRAD_DIRECT_RG, K_WGRAD_DIRECT_CPS_RG},
                                             {K_WGRAD_DIRECT_F16_RG, K_WGRAD_DIRECT_F16_CPS_RG}};
constexpr StepKernel kWgradDirectCpsS16[2] = {K_WGRAD_DIRECT_CPS_S16, K_WGRAD_DIRECT_F16_CPS_S16};

// The launches of a step in their order: the exact entry point of each, and its grid (0: not made).
struct StepPlan {
  int splits, max_splits;       // this step's split-K factor; the one its workspace is laid out for
  StepKernel prep;
  int prep_grid;                // standalone dad_prep of this step's rows before the encoder (all parts); 0: none
  StepKernel encode;
  int encode_grid, ws_nt, ws_ns;   // (ws_nt / ws_ns: dad_encode_wp's roles; encode_rc: wp_split's code)
  int encode_rc;
  StepKernel pool;
  int pool_grid;                // the separate dad_pool; 0: the tail launch pools
  StepKernel tail;
  int tail_grid;
  int tail_prep;                // DAD_PREP_* parts of the NEXT batch the tail launch prepares
  // the supervised-contrastive term's four launches (scl.hip), between the tail and the weight gradient; scl_n = 0:
  // not made.  Not among the DAD_STEP_LAUNCHES dad_step_plan_kernels lists: dad_scl_plan reports this grid.
  int scl_n;
  SclPlan scl;
  StepKernel wgrad;
  int wgrad_grid, wgrad_tiles;
  int wgrad_clean, wgrad_store;    // it converts the next batch's clean rows; through that batch's store table
  StepKernel reduce;
  int reduce_grid;
  int prepped, pending;         // as dad_step_backward_ahead_split reports them
};

// The next step's batch may be prepared in this step's launches when the tail runs as
// dad_tail_ecda_w and the next step has this step's workspace layout (so its prepared set sits
// where the next step will look) and the other set parity.
inline bool can_prepare_ahead(const dad_config* cfg, int max_splits, const dad_config* ncfg, const dad_batch* nbt) {
  if (!ncfg || !nbt || check_cfg(ncfg) != DAD_OK) return false;
  if (!dad_prec16(cfg->precision) || ncfg->precision != cfg->precision) return false;
  if (ncfg->B != cfg->B || ncfg->T != cfg->T || ncfg->Bn != cfg->Bn || ncfg->Tn != cfg->Tn) return false;
  if (((ncfg->counter ^ cfg->counter) & 1u) == 0) return false;
  if (max_splits_of(ncfg) != max_splits) return false;
  // a set prepared ragged holds its live rows only: a ragged step reads it, and a dense step a dense set
  if ((ncfg->ragged != 0) != (cfg->ragged != 0) || check_ragged_batch(ncfg, nbt) != DAD_OK) return false;
  // (a store of any DAD_STORE_* type qualifies: the preparation reads 16-bit rows in place; the callers
  // report check_batch_dtypes' code for a batch it refuses)
  if (check_batch_dtypes(ncfg, nbt) != DAD_OK) return false;
  if (!nbt->xc || !nbt->mc) return false;
  if (!ncfg->warmup && (!nbt->xn || !nbt->mn)) return false;
  if (ncfg->rng_mode == DAD_RNG_EXPLICIT && !ncfg->warmup && !has_explicit_draws(nbt)) return false;
  return rows_paired(nbt);
}

// cfg: a config check_cfg accepts.  (next_cfg, next_batch): the step after it, or NULL; one that does
// not qualify (can_prepare_ahead) is prepared by its own step.  defer: the DAD_PREP_* parts of the
// next batch's rows this step's launches leave to the caller (dad_step_prepare_rows).  cus: the
// device's compute units.  batch: this step's, or NULL for a padded f32 one; of it and of next_batch
// only the struct's own fields are read (NULL-ness of pointers, xc_dtype / xn_dtype).
inline StepPlan plan_step(const dad_config* cfg, const dad_batch* batch, const dad_config* next_cfg,
                          const dad_batch* next_batch, int defer, int cus) {
  StepPlan p = {};
  const DadGeom G = geom_of(cfg);
  const int Bn = cfg->warmup ? 0 : G.Bn;
  const bool h16 = dad_prec16(cfg->precision), f16 = cfg->precision == DAD_PREC_FP16, ragged = cfg->ragged != 0;
  p.splits = splits_of(cfg);
  p.max_splits = max_splits_of(cfg);

  // encoder.  16-bit: augmentation + conversion (unless the previous step prepared this batch),
  // then the W-stationary GEMM on the prepared set.  FP32: one wave per 32-row slab, four per
  // workgroup.
  p.prep = prep_kernel(ragged, rows_need_s16(cfg, batch, DAD_PREP_CLEAN | DAD_PREP_NOISY));
  p.encode = encode_kernel(cfg->precision, ragged);
  if (h16) {
    if (!cfg->prepped) p.prep_grid = prep_grid_of(cus);
    p.encode_rc = wp_split(G, Bn, cus, p.ws_nt, p.ws_ns);
    p.encode_grid = p.ws_nt + p.ws_ns;
  } else {
    p.encode_grid = (G.Bc * G.ncc + Bn * G.ncn + 3) / 4;
  }

  // pooling and tail.  Batches of at most 64 utterances per side with class-aware MMD, after the
  // warm-up: the wave-centric launch, whose spare blocks pool the embeddings (one item per wave,
  // Bc + 2 Bn items) instead of a separate dad_pool launch.  Warm-up: no ECDA.  Otherwise block 0 is
  // the tail and blocks 1..C the classes.  (A ragged step pools live slabs only, in dad_pool_rg or in
  // dad_tail_ecda_w_rg; dad_tail and dad_tail_ecda do not pool and have no sibling.)
  const bool tail_w = !cfg->warmup && G.Bc <= 64 && Bn <= 64 && cfg->class_aware && tail_w_on();
  const int items = G.Bc + 2 * Bn, waves = DAD_TAIL_THREADS / 64;
  p.pool = ragged ? K_POOL_RG : K_POOL;
  if (!tail_w) p.pool_grid = items;
  p.tail = cfg->warmup ? K_TAIL : tail_w ? K_TAIL_ECDA_W : K_TAIL_ECDA;
  p.tail_grid = cfg->warmup ? 1 : 1 + DAD_C + (tail_w ? (items + waves - 1) / waves : 0);

  // preparation ahead: the next batch's clean rows in the weight-gradient launch (interleaved with
  // the GEMM), its noisy rows on the CUs the tail and class blocks leave idle
  if (tail_w && can_prepare_ahead(cfg, p.max_splits, next_cfg, next_batch)) {
    p.prepped = 1;
    p.pending = defer & (DAD_PREP_CLEAN | DAD_PREP_NOISY);
    p.wgrad_clean = !(defer & DAD_PREP_CLEAN);
    p.wgrad_store = p.wgrad_clean && next_batch->rowc != nullptr;
    p.tail_prep = (defer & DAD_PREP_NOISY) ? 0 : DAD_PREP_NOISY;
    if (p.tail_prep) p.tail_grid = std::max(p.tail_grid, std::max(cus, 2 * (1 + DAD_C)));
  }
  // (the `_s16` tail: when the rows it prepares lie in a 16-bit store)
  if (tail_w && ragged) p.tail = K_TAIL_ECDA_W_RG;
  else if (p.tail_prep && rows_need_s16(next_cfg, next_batch, p.tail_prep)) p.tail = K_TAIL_ECDA_W_S16;

  // the supervised-contrastive term: the clean rows and the strong rows as one set of Bc + Bn
  if (scl_in_step(cfg)) {
    p.scl_n = G.Bc + Bn;
    p.scl = scl_plan_of(p.scl_n, cus);
  }

  // weight gradient and the split sums.  16-bit: WGD_NDB column blocks per split, the grid a
  // multiple of 8 (XCD-aware tile order) with WGD_XWG spare workgroups for the reduce's extra blocks.
  // FP32: one tile = (split, 128 columns); then every reduce block.
  if (h16) {
    if (ragged) p.wgrad = kWgradDirectRg[f16][p.wgrad_clean];
    else if (p.wgrad_store && next_batch->xc_dtype != DAD_STORE_F32) p.wgrad = kWgradDirectCpsS16[f16];
    else p.wgrad = kWgradDirect[f16][p.wgrad_clean][p.wgrad_store];
    p.wgrad_tiles = WGD_NDB * p.splits;
    p.wgrad_grid = (p.wgrad_tiles + WGD_XWG + 7) / 8 * 8;
    p.reduce = K_REDUCE_W;
    p.reduce_grid = DAD_REDUCE_BLOCKS - DAD_REDUCE_XBLK;
  } else {
    p.wgrad = K_WGRAD_F32;
    p.wgrad_tiles = p.wgrad_grid = 6 * p.splits;
    p.reduce = K_REDUCE;
    p.reduce_grid = DAD_REDUCE_BLOCKS;
  }
  return p;
}

// dad_step_ragged_plan (dad.h): the shares of a ragged step's live slabs, from host copies of the lengths,
// by the functions the `_rg` kernels call on the device lengths (dad_common.h "Ragged mode"): the encoder's
// grid is wp_split's and the split count splits_of's, as for the dense step (neither depends on the
// lengths).  (A diagnostic: it allocates its three prefix arrays.)
inline int ragged_plan(const dad_config* cfg, const int32_t* lenc, const int32_t* lenn, int cus, dad_ragged_plan* out) {
  const DadGeom G = geom_of(cfg);
  const int Bn = cfg->warmup ? 0 : G.Bn, n = G.Bc + Bn;
  int nt = 0, ns = 0;
  const int rc = wp_split(G, Bn, cus, nt, ns);
  if (rc) return rc;
  const int splits = splits_of(cfg);
  out->enc_grid = nt + ns;
  out->splits = splits;
  if (!out->enc || !out->split || out->enc_capacity < nt + ns || out->split_capacity < splits) return DAD_E_ARG;
  std::vector<int> pre(3 * (size_t)(n + 1));
  int* ps = pre.data();
  int* pss = ps + (n + 1);
  int* pz = pss + (n + 1);
  dad_live_prefix_host(lenc, G.Bc, G.ncc, G.Tc, lenn, Bn, G.ncn, G.Tn, ps, pss, pz);
  out->live_clean = ps[G.Bc];
  out->live_noisy = ps[n] - ps[G.Bc];
  out->max_enc_range = 0;
  const bool by_t = dad_rg_by_slabs(nt, ns, ps, pss, G.Bc, n, true, DAD_ENC_WS_MAXJ);
  const bool by_s = dad_rg_by_slabs(nt, ns, ps, pss, G.Bc, n, false, DAD_ENC_WS_MAXJ);
  for (int wg = 0; wg < nt + ns; ++wg) {
    bool t = false;
    int j0 = 0, j1 = 0;
    dad_rg_job_range(wg, nt, ns, ps, pss, G.Bc, n, wg < nt ? by_t : by_s, t, j0, j1);
    out->enc[3 * wg] = t ? 1 : 0;
    out->enc[3 * wg + 1] = j0;
    out->enc[3 * wg + 2] = j1 - j0;
    out->max_enc_range = std::max(out->max_enc_range, j1 - j0);
  }
  out->max_split_utts = 0;
  for (int s = 0; s < splits; ++s) {
    int s0 = 0, s1 = 0;
    dad_wg_share(ps[n], splits, s, s0, s1);
    out->split[2 * s] = s0;
    out->split[2 * s + 1] = s1;
    if (s0 < s1)
      out->max_split_utts = std::max(out->max_split_utts, pz[dad_live_find(ps, n, s1 - 1)] - pz[dad_live_find(ps, n, s0)] + 1);
  }
  return DAD_OK;
}
