// Host side of the C ABI (include/dad.h): argument validation, workspace carving and the
// kernel sequence of one DAD step, as step_plan.h plans it.  Enqueue-only: no allocation, no
// synchronisation.
#include <string.h>

#include "dad_host.h"
#include "dad_timing.h"

constexpr int kMaxDevices = 64;

int device_cus(int* out) {
  static int cache[kMaxDevices];
  int dev = 0;
  DAD_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return DAD_E_ARG;
  if (!cache[dev]) DAD_TRY(hipDeviceGetAttribute(&cache[dev], hipDeviceAttributeMultiprocessorCount, dev));
  *out = cache[dev];
  return DAD_OK;
}

namespace {

inline DadStoreRows store_rows_of(const dad_batch* bt) { return DadStoreRows{bt->rowc, bt->lenc, bt->rown, bt->lenn}; }

// Row-preparation arguments (dad_prep.h) of the step described by (cfg, bt) into set x16.
DadPrepArgs prep_args(const dad_config* cfg, const dad_batch* bt, uint16_t* x16) {
  DadPrepArgs p;
  memset(&p, 0, sizeof(p));
  const Keys k = keys_of(cfg);
  p.g = geom_of(cfg);
  p.warmup = cfg->warmup; p.mask_len = cfg->mask_len; p.start_hi = cfg->start_hi;
  p.f16 = cfg->precision == DAD_PREC_FP16 ? 1 : 0;
  p.clean = 1;
  p.xc = bt->xc; p.xn = bt->xn;
  p.src = store_rows_of(bt);
  p.src_types = bt->xc_dtype | (bt->xn_dtype << 8);   // (check_batch_dtypes: F32 for a padded batch)
  if (cfg->rng_mode == DAD_RNG_EXPLICIT) { p.nw = bt->nw; p.ns = bt->ns; p.u = bt->u; p.start = bt->start; }
  p.key_weak = k.weak; p.key_strong = k.strong; p.key_feat = k.feat; p.key_tstart = k.tstart;
  p.weak_std = cfg->weak_std; p.strong_std = cfg->strong_std; p.feat_p = cfg->feat_p;
  p.x16 = x16;
  return p;
}

// the step's arguments: config, and every pointer its kernels follow
int check_step_args(const dad_config* cfg, const dad_batch* bt, const dad_state* st, const void* workspace) {
  const int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!bt || !st || !workspace) return DAD_E_ARG;
  if (!bt->xc || !bt->mc || !bt->yc || !st->student || !st->teacher || !st->grad || !st->dacp || !st->tail ||
      !st->emb || !st->logits || !st->w1bf_student || !st->w1bf_teacher)
    return DAD_E_ARG;
  if (!cfg->warmup && (!bt->xn || !bt->mn)) return DAD_E_ARG;
  const bool explicit_rng = cfg->rng_mode == DAD_RNG_EXPLICIT;
  if (explicit_rng && cfg->p_drop > 0.0f && (!bt->keep1 || (!cfg->warmup && !bt->keep2))) return DAD_E_ARG;
  if (explicit_rng && !cfg->warmup && !has_explicit_draws(bt)) return DAD_E_ARG;
  if (!rows_paired(bt)) return DAD_E_ARG;
  const int rrc = check_ragged_batch(cfg, bt);
  if (rrc) return rrc;
  return check_batch_dtypes(cfg, bt);
}

// the next batch a step may prepare (or NULL): one whose row types the step cannot read is an error,
// not a batch left to its own step
int check_next_batch(const dad_config* ncfg, const dad_batch* nbt) {
  if (!ncfg || !nbt || check_cfg(ncfg) != DAD_OK) return DAD_OK;
  return check_batch_dtypes(ncfg, nbt);
}

// dad_step_plan / dad_step_plan_kernels: their arguments checked, then the plan the step enqueues from
int plan_query(const dad_config* cfg, const dad_batch* batch, const dad_config* next_cfg, const dad_batch* next_batch,
               int defer, int cus, bool has_out, StepPlan* plan) {
  const int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cus < 2 || !has_out || (defer & ~(DAD_PREP_CLEAN | DAD_PREP_NOISY)) != 0) return DAD_E_ARG;
  const int brc = batch ? check_batch_dtypes(cfg, batch) : DAD_OK;
  if (brc) return brc;
  const int nrc = check_next_batch(next_cfg, next_batch);
  if (nrc) return nrc;
  *plan = plan_step(cfg, batch, next_cfg, next_batch, defer, cus);
  return plan->encode_rc;
}

// p restricted to `parts` (DAD_PREP_*) of its set
void prep_only(DadPrepArgs& p, int parts) {
  p.clean = (parts & DAD_PREP_CLEAN) ? 1 : 0;
  if (!(parts & DAD_PREP_NOISY)) p.warmup = 1;   // (dad_prep_rows: no noisy rows in a warm-up set)
}

// The regions of a step's workspace (dad_ws_layout), carved once.
struct StepWs {
  float *part_sum, *part_cnt, *vlen, *cnt_tot, *ge, *ge_ecda, *normpart, *ecda, *gzb, *gflat, *wpart;
  uint32_t *bits, *eflag, *pool_ready;
  // 16-bit modes: the two prepared sets.  A step reads the one of its counter's parity; the next step's
  // is the other one, so preparing it in this step's launches leaves this one intact for wgrad.
  uint16_t* x16[2];
  StepWs(void* ws, const DadWs& L)
      : part_sum(ws_ptr<float>(ws, L.part_sum)), part_cnt(ws_ptr<float>(ws, L.part_cnt)),
        vlen(ws_ptr<float>(ws, L.vlen)), cnt_tot(ws_ptr<float>(ws, L.cnt_tot)), ge(ws_ptr<float>(ws, L.ge)),
        ge_ecda(ws_ptr<float>(ws, L.ge_ecda)), normpart(ws_ptr<float>(ws, L.normpart)),
        ecda(ws_ptr<float>(ws, L.ecda)), gzb(ws_ptr<float>(ws, L.gzb)), gflat(ws_ptr<float>(ws, L.gflat)),
        wpart(ws_ptr<float>(ws, L.wpart)), bits(ws_ptr<uint32_t>(ws, L.bits)), eflag(ws_ptr<uint32_t>(ws, L.eflag)),
        pool_ready(ws_ptr<uint32_t>(ws, L.ready)),
        x16{ws_ptr<uint16_t>(ws, L.xs16), ws_ptr<uint16_t>(ws, L.xs16 + L.x16set)} {}
  uint16_t* set_of(const dad_config* c) const { return x16[c->counter & 1u]; }
};

// What the argument blocks of one step are filled from.
struct Step {
  const dad_config* cfg;
  const dad_batch* bt;
  const dad_state* st;
  const StepPlan& plan;
  DadGeom G;
  Keys k;
  StepWs ws;
  Step(const dad_config* c, const dad_batch* b, const dad_state* s, const StepPlan& p, void* workspace)
      : cfg(c), bt(b), st(s), plan(p), G(geom_of(c)), k(keys_of(c)),
        ws(workspace, dad_ws_layout(G, p.max_splits, c->precision)) {}
  bool explicit_rng() const { return cfg->rng_mode == DAD_RNG_EXPLICIT; }
};

// 1. fused augmentation + encoder GEMMs + pooling partials
DadEncodeArgs encode_args(const Step& s) {
  const dad_config* cfg = s.cfg;
  const dad_batch* bt = s.bt;
  DadEncodeArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.g = s.G; ea.warmup = cfg->warmup;
  ea.mask_len = cfg->mask_len; ea.start_hi = cfg->start_hi;
  // (the FP32 encoder reads the rows, f32 by check_batch_dtypes; the 16-bit ones read the prepared set)
  ea.xc = static_cast<const float*>(bt->xc); ea.mc = bt->mc; ea.xn = static_cast<const float*>(bt->xn); ea.mn = bt->mn;
  ea.src = store_rows_of(bt);
  ea.w1_student = s.st->student + DAD_OFF_W1; ea.b1_student = s.st->student + DAD_OFF_B1;
  ea.w1_teacher = s.st->teacher + DAD_OFF_W1; ea.b1_teacher = s.st->teacher + DAD_OFF_B1;
  ea.w1h_student = s.st->w1bf_student;
  ea.w1h_teacher = s.st->w1bf_teacher;
  ea.pool_ready = s.ws.pool_ready;
  if (s.explicit_rng()) { ea.nw = bt->nw; ea.ns = bt->ns; ea.u = bt->u; ea.start = bt->start; }
  ea.key_weak = s.k.weak; ea.key_strong = s.k.strong; ea.key_feat = s.k.feat; ea.key_tstart = s.k.tstart;
  ea.weak_std = cfg->weak_std; ea.strong_std = cfg->strong_std; ea.feat_p = cfg->feat_p;
  ea.part_sum = s.ws.part_sum; ea.part_cnt = s.ws.part_cnt; ea.bits = s.ws.bits;
  ea.ws_nt = s.plan.ws_nt; ea.ws_ns = s.plan.ws_ns;
  const size_t nrc = (size_t)s.G.Bc * s.G.Tc, nrn = (size_t)s.G.Bn * s.G.Tn;
  ea.x16c = s.ws.set_of(cfg); ea.x16s = ea.x16c + nrc * DAD_D; ea.x16w = ea.x16s + (cfg->warmup ? 0 : nrn) * DAD_D;
  return ea;
}

// 2. pooled embeddings + classifier logits: a launch of its own, or the spare blocks of the
//    wave-centric tail launch (pa.ready: its arrival counters, zeroed by this step's encoder)
DadPoolArgs pool_args(const Step& s) {
  const dad_config* cfg = s.cfg;
  const dad_batch* bt = s.bt;
  DadPoolArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.g = s.G; pa.warmup = cfg->warmup;
  pa.mc = bt->mc; pa.mn = bt->mn; pa.part_sum = s.ws.part_sum;
  pa.student = s.st->student; pa.teacher = s.st->teacher;
  if (s.explicit_rng()) { pa.keep1 = bt->keep1; pa.keep2 = bt->keep2; }
  pa.key_drop1 = s.k.drop1; pa.key_drop2 = s.k.drop2;
  pa.p_drop = cfg->p_drop; pa.drop_scale = cfg->drop_scale;
  pa.emb = s.st->emb; pa.vlen = s.ws.vlen; pa.logits = s.st->logits;
  pa.part_cnt = s.ws.part_cnt; pa.cnt_tot = s.ws.cnt_tot;
  pa.eflag = s.ws.eflag; pa.tail_terms = s.st->tail + DAD_T_ECDA_TERM;
  pa.range_flag = reinterpret_cast<uint32_t*>(s.st->tail + DAD_T_RANGE);
  if (cfg->ragged) { pa.lenc = bt->lenc; pa.lenn = bt->lenn; }
  if (!s.plan.pool_grid) pa.ready = s.ws.pool_ready;
  return pa;
}

// 3. losses, DACP mask, analytic backward to dL/de and the classifier grads
DadTailArgs tail_args(const Step& s) {
  DadTailArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.cfg = *s.cfg; ta.yc = s.bt->yc; ta.logits = s.st->logits; ta.emb = s.st->emb; ta.student = s.st->student;
  if (s.explicit_rng()) { ta.keep1 = s.bt->keep1; ta.keep2 = s.bt->keep2; }
  ta.key_drop1 = s.k.drop1; ta.key_drop2 = s.k.drop2;
  ta.dacp = s.st->dacp; ta.tailf = s.st->tail; ta.ge = s.ws.ge; ta.ge_ecda = s.ws.ge_ecda; ta.grad = s.st->grad;
  ta.gzb = s.ws.gzb; ta.eflag = s.ws.eflag;
  return ta;
}

// 4. ECDA (class-aware MMD + compactness + repulsion) and its embedding grads: after the
//    warm-up, in the same launch as the tail (block 0 = tail, blocks 1..C = classes)
DadEcdaArgs ecda_args(const Step& s) {
  DadEcdaArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.cfg = *s.cfg; ca.yc = s.bt->yc; ca.emb = s.st->emb; ca.tailf = s.st->tail;
  ca.tail_terms = s.st->tail + DAD_T_ECDA_TERM; ca.ge = s.ws.ge_ecda; ca.scratch = s.ws.ecda; ca.eflag = s.ws.eflag;
  ca.sink = s.ws.gflat;
  return ca;
}

// 5. dW1 as one direct split-K GEMM (G = ReLU' * dL/de / len rebuilt from the tail's dL/dz
//    and the ECDA rows), then the split sums with db1, dW2, loss totals, squared-norm partials
DadWgradArgs wgrad_args(const Step& s) {
  const dad_config* cfg = s.cfg;
  const dad_batch* bt = s.bt;
  DadWgradArgs wa;
  memset(&wa, 0, sizeof(wa));
  wa.g = s.G; wa.warmup = cfg->warmup;
  wa.mask_len = cfg->mask_len; wa.start_hi = cfg->start_hi;
  wa.xc = static_cast<const float*>(bt->xc); wa.xn = static_cast<const float*>(bt->xn);   // (FP32 only)
  wa.src = store_rows_of(bt);
  if (s.explicit_rng()) { wa.ns = bt->ns; wa.u = bt->u; wa.start = bt->start; }
  wa.key_strong = s.k.strong; wa.key_feat = s.k.feat; wa.key_tstart = s.k.tstart;
  wa.strong_std = cfg->strong_std; wa.feat_p = cfg->feat_p;
  wa.bits = s.ws.bits; wa.ge = s.ws.ge; wa.vlen = s.ws.vlen; wa.xs16 = s.ws.set_of(cfg);
  wa.splits = s.plan.splits; wa.ntiles = s.plan.wgrad_tiles;
  wa.wpart = s.ws.wpart;
  return wa;
}

DadReduceArgs reduce_args(const Step& s) {
  const dad_config* cfg = s.cfg;
  DadReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.g = s.G; ra.warmup = cfg->warmup;
  ra.want_norm = cfg->dp_world == 1;
  ra.w_kl = cfg->w_kl; ra.w_ecda = cfg->w_ecda;
  ra.w_scl = s.plan.scl_n ? cfg->w_scl : 0.0f;
  ra.ge_ecda = s.ws.ge_ecda;
  ra.gzb = s.ws.gzb; ra.eflag = s.ws.eflag; ra.student = s.st->student; ra.emb = s.st->emb;
  if (s.explicit_rng()) { ra.keep1 = s.bt->keep1; ra.keep2 = s.bt->keep2; }
  ra.key_drop1 = s.k.drop1; ra.key_drop2 = s.k.drop2; ra.p_drop = cfg->p_drop; ra.drop_scale = cfg->drop_scale;
  ra.ge = s.ws.ge; ra.vlen = s.ws.vlen; ra.cnt_tot = s.ws.cnt_tot; ra.tailf = s.st->tail;
  ra.grad = s.st->grad; ra.normpart = s.ws.normpart;
  ra.pool_abort = s.plan.pool_grid ? nullptr : s.ws.pool_ready + DAD_POOL_ABORT;
  ra.splits = s.plan.splits; ra.wpart = s.ws.wpart;
  return ra;
}

// The tail and the weight gradient, each with the argument blocks its kernel's class takes.
int launch_tail(const Step& s, hipStream_t stream, const DadPrepArgs& next_rows, const DadPoolArgs& pa) {
  const StepPlan& p = s.plan;
  switch (kStepKernels[p.tail].sig) {
    case SIG_TAIL: return launch(p.tail, p.tail_grid, stream, tail_args(s));
    case SIG_TAIL_ECDA: return launch(p.tail, p.tail_grid, stream, tail_args(s), ecda_args(s));
    default: return launch(p.tail, p.tail_grid, stream, tail_args(s), ecda_args(s), next_rows, pa);
  }
}
int launch_wgrad(const Step& s, hipStream_t stream, const DadPrepArgs& next_clean, const DadReduceArgs& ra) {
  const StepPlan& p = s.plan;
  if (kStepKernels[p.wgrad].sig == SIG_WGRAD_CP) return launch(p.wgrad, p.wgrad_grid, stream, wgrad_args(s), ra, next_clean);
  return launch(p.wgrad, p.wgrad_grid, stream, wgrad_args(s), ra);
}

// The workspace of a step: dad_ws_layout's regions, then (dad_config.scl_on) dad_scl's workspace for the Bc + Bn
// rows, so a step without the term has the layout and the size it had.
size_t step_ws_bytes(const dad_config* cfg) {
  const size_t base = dad_ws_layout(geom_of(cfg), max_splits_of(cfg), cfg->precision).bytes;
  return cfg->scl_on ? dad_align(base) + scl_ws_bytes(cfg->B + (cfg->Bn > 0 ? cfg->Bn : 0)) : base;
}

// 3b. the supervised-contrastive term on what the tail launch left: the clean rows with their labels and the strong
//     rows the DACP mask lets in with the teacher's pseudo-labels; the loss into the tail buffer, w_scl dL/de into
//     the ECDA rows of dL/de (flagging the rows it writes, as ECDA does: the fused weight gradient adds flagged rows)
int launch_scl(const Step& s, void* workspace, hipStream_t stream) {
  const dad_config* cfg = s.cfg;
  const int B = s.G.Bc, Bn = s.G.Bn;
  float* tail = s.st->tail;
  const SclSrc src{s.st->emb, s.bt->yc, nullptr, B,
                   s.st->emb + (size_t)(B + Bn) * DAD_H, tail + DAD_TAIL_HDR + Bn, tail + DAD_TAIL_HDR + 2 * Bn, Bn};
  const SclDst dst{nullptr, tail + DAD_T_SCL, nullptr, s.ws.ge_ecda, s.ws.eflag, cfg->w_scl};
  const size_t off = dad_align(dad_ws_layout(s.G, s.plan.max_splits, cfg->precision).bytes);
  return scl_enqueue(src, dst, cfg->scl_tau, s.plan.scl, ws_ptr<char>(workspace, off), stream);
}

}  // namespace

extern "C" {

int dad_abi_version(void) { return DAD_ABI_VERSION; }
size_t dad_param_count(void) { return DAD_NPARAM; }

const char* dad_error_string(int code) {
  switch (code) {
    case DAD_OK: return "ok";
    case DAD_E_ARG: return "DAD_E_ARG: invalid argument";
    case DAD_E_SHAPE: return "DAD_E_SHAPE: unsupported batch/sequence shape";
    case DAD_E_COMM: return "DAD_E_COMM: RCCL failure";
    case DAD_E_UNSUPPORTED: return "DAD_E_UNSUPPORTED";
    default: return hipGetErrorString((hipError_t)code);
  }
}

int dad_encoder_ws_plan(const dad_config* cfg, int cus, int* nt, int* ns, int* max_jobs) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cus < 2 || !nt || !ns || !max_jobs) return DAD_E_ARG;
  const DadGeom G = geom_of(cfg);
  const int Bn = cfg->warmup ? 0 : G.Bn;
  rc = wp_split(G, Bn, cus, *nt, *ns);
  if (rc) return rc;
  *max_jobs = wp_max_range(G, Bn, *nt, *ns);
  return DAD_OK;
}

int dad_encoder_ws_jobs(const dad_config* cfg, int cus, int* jobs, int capacity) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cus < 2 || !jobs) return DAD_E_ARG;
  const DadGeom G = geom_of(cfg);
  const int Bn = cfg->warmup ? 0 : G.Bn;
  int nt = 0, ns = 0;
  rc = wp_split(G, Bn, cus, nt, ns);
  if (rc) return rc;
  if (capacity < 4 * (nt + ns)) return DAD_E_ARG;   // the grid outgrew the caller's table
  for (int wg = 0; wg < nt + ns; ++wg) {
    bool t = false;
    int j0 = 0, j1 = 0;
    dad_wp_job_range(wg, nt, ns, G.Bc, G.Tc, G.ncc, Bn, G.Tn, G.ncn, Bn * G.ncn, t, j0, j1);
    jobs[4 * wg] = t ? 1 : 0;
    jobs[4 * wg + 1] = j0;
    jobs[4 * wg + 2] = 1;
    jobs[4 * wg + 3] = j1 - j0;
  }
  return nt + ns;
}

int dad_step_plan(const dad_config* cfg, const dad_config* next_cfg, const dad_batch* next_batch, int defer, int cus,
                  dad_step_plan_info* out) {
  StepPlan p;
  const int rc = plan_query(cfg, nullptr, next_cfg, next_batch, defer, cus, out != nullptr, &p);
  if (rc) return rc;
  *out = dad_step_plan_info{p.splits, p.max_splits, p.prep_grid, p.encode_grid, p.ws_nt, p.ws_ns, p.pool_grid,
                            p.tail_grid, p.tail_prep, p.tail_prep == DAD_PREP_CLEAN, p.wgrad_grid, p.wgrad_clean,
                            p.wgrad_store, p.reduce_grid, p.prepped, p.pending, family_name(p.encode),
                            family_name(p.tail), family_name(p.wgrad), family_name(p.reduce)};
  return DAD_OK;
}

int dad_step_plan_kernels(const dad_config* cfg, const dad_batch* batch, const dad_config* next_cfg,
                          const dad_batch* next_batch, int defer, int cus, const char* out[DAD_STEP_LAUNCHES]) {
  StepPlan p;
  const int rc = plan_query(cfg, batch, next_cfg, next_batch, defer, cus, out != nullptr, &p);
  if (rc) return rc;
  const struct { StepKernel kernel; int grid; } launches[DAD_STEP_LAUNCHES] = {
      {p.prep, p.prep_grid}, {p.encode, p.encode_grid}, {p.pool, p.pool_grid},
      {p.tail, p.tail_grid}, {p.wgrad, p.wgrad_grid}, {p.reduce, p.reduce_grid}};
  for (int i = 0; i < DAD_STEP_LAUNCHES; ++i) out[i] = launches[i].grid ? kStepKernels[launches[i].kernel].name : nullptr;
  return DAD_OK;
}

int dad_step_ragged_plan(const dad_config* cfg, const int32_t* lenc, const int32_t* lenn, int cus, dad_ragged_plan* out) {
  const int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!dad_prec16(cfg->precision)) return DAD_E_UNSUPPORTED;
  if (cus < 2 || !out || !lenc || (!cfg->warmup && !lenn)) return DAD_E_ARG;
  return ragged_plan(cfg, lenc, lenn, cus, out);
}

int dad_workspace_bytes(const dad_config* cfg, size_t* bytes) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!bytes) return DAD_E_ARG;
  *bytes = step_ws_bytes(cfg);
  return DAD_OK;
}

}  // extern "C"

// dad_step_backward_ahead[_split]'s request: the next step, the DAD_PREP_* parts of its rows left to the
// caller, and where to report what was enqueued
struct Ahead {
  const dad_config* cfg;
  const dad_batch* batch;
  int defer;
  int* prepped;
  int* pending;
};

// The launches of one step: validate, plan (step_plan.h), carve the workspace, fill the argument blocks,
// launch what the plan says in its order.
static int step_compute_phases(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                               void* stream_, bool do_encode, bool do_backward, const Ahead& ahead = Ahead{}) {
  if (ahead.prepped) *ahead.prepped = 0;
  if (ahead.pending) *ahead.pending = 0;
  int rc = check_step_args(cfg, bt, st, workspace);
  if (rc) return rc;
  rc = check_next_batch(ahead.cfg, ahead.batch);
  if (rc) return rc;
  int cus = 0;
  rc = device_cus(&cus);
  if (rc) return rc;
  const StepPlan plan = plan_step(cfg, bt, ahead.cfg, ahead.batch, ahead.defer, cus);
  const Step s(cfg, bt, st, plan, workspace);
  hipStream_t stream = (hipStream_t)stream_;

  if (do_encode) {
    if (plan.encode_rc) return plan.encode_rc;
    tk_begin();
    tk_mark(TK_E0, stream);
    if (plan.prep_grid) DAD_RET(launch(plan.prep, plan.prep_grid, stream, prep_args(cfg, bt, s.ws.set_of(cfg))));
    DAD_RET(launch(plan.encode, plan.encode_grid, stream, encode_args(s)));
    tk_mark(TK_E1, stream);
  }
  if (!do_backward) return DAD_OK;
  if (ahead.prepped) *ahead.prepped = plan.prepped;
  if (ahead.pending) *ahead.pending = plan.pending;

  // (no pool timing point when the tail launch pools: that launch is timed from the encoder's end)
  const DadPoolArgs pa = pool_args(s);
  if (plan.pool_grid) {
    DAD_RET(launch(plan.pool, plan.pool_grid, stream, pa));
    tk_mark(TK_POOL, stream);
  }
  // the next batch's rows this step prepares: in the tail launch, and (its clean rows) in the
  // weight-gradient launch; x16 = NULL: nothing
  DadPrepArgs in_tail, in_wgrad;
  memset(&in_tail, 0, sizeof(in_tail));
  memset(&in_wgrad, 0, sizeof(in_wgrad));
  if (plan.prepped) {
    const DadPrepArgs next = prep_args(ahead.cfg, ahead.batch, s.ws.set_of(ahead.cfg));
    if (plan.wgrad_clean) in_wgrad = next;
    if (plan.tail_prep) { in_tail = next; prep_only(in_tail, plan.tail_prep); }
  }
  DAD_RET(launch_tail(s, stream, in_tail, pa));
  if (plan.scl_n) DAD_RET(launch_scl(s, workspace, stream));   // (timed with the tail: DAD_TK_TAIL)
  tk_mark(TK_TAIL, stream);
  const DadReduceArgs ra = reduce_args(s);
  DAD_RET(launch_wgrad(s, stream, in_wgrad, ra));
  tk_mark(TK_WGRAD, stream);
  DAD_RET(launch(plan.reduce, plan.reduce_grid, stream, ra));
  tk_mark(TK_RED, stream);
  return DAD_OK;
}

extern "C" {

int dad_step_compute(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                     void* stream) {
  return step_compute_phases(cfg, bt, st, workspace, stream, true, true);
}

int dad_step_encode(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                    void* stream) {
  return step_compute_phases(cfg, bt, st, workspace, stream, true, false);
}

int dad_step_backward(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                      void* stream) {
  return step_compute_phases(cfg, bt, st, workspace, stream, false, true);
}

int dad_step_backward_ahead(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                            void* stream, const dad_config* next_cfg, const dad_batch* next_batch, int* prepped) {
  return step_compute_phases(cfg, bt, st, workspace, stream, false, true, Ahead{next_cfg, next_batch, 0, prepped, nullptr});
}

int dad_step_backward_ahead_split(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                                  void* stream, const dad_config* next_cfg, const dad_batch* next_batch, int defer,
                                  int* prepped, int* pending) {
  if (!pending || (defer & ~(DAD_PREP_CLEAN | DAD_PREP_NOISY)) != 0) return DAD_E_ARG;
  return step_compute_phases(cfg, bt, st, workspace, stream, false, true,
                             Ahead{next_cfg, next_batch, defer, prepped, pending});
}

int dad_step_prepare_rows(const dad_config* cfg, const dad_batch* bt, void* workspace, void* stream, int parts) {
  const int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!bt || !workspace || (parts & ~(DAD_PREP_CLEAN | DAD_PREP_NOISY)) != 0) return DAD_E_ARG;
  if (!dad_prec16(cfg->precision)) return DAD_E_UNSUPPORTED;
  if (parts == 0) return DAD_OK;
  // only the parts asked for need their pointers: xc for the clean rows; xn and the draws for the noisy ones
  if ((parts & DAD_PREP_CLEAN) && !bt->xc) return DAD_E_ARG;
  if (cfg->warmup) parts &= ~DAD_PREP_NOISY;   // (a warm-up set has no noisy rows)
  if ((parts & DAD_PREP_NOISY) && (!bt->xn || (cfg->rng_mode == DAD_RNG_EXPLICIT && !has_explicit_draws(bt))))
    return DAD_E_ARG;
  if (!rows_paired(bt)) return DAD_E_ARG;
  if (cfg->ragged && (((parts & DAD_PREP_CLEAN) && !bt->lenc) || ((parts & DAD_PREP_NOISY) && !bt->lenn))) return DAD_E_ARG;
  const int drc = check_batch_dtypes(cfg, bt);
  if (drc) return drc;
  if (parts == 0) return DAD_OK;
  const DadWs L = dad_ws_layout(geom_of(cfg), max_splits_of(cfg), cfg->precision);
  DadPrepArgs p = prep_args(cfg, bt, ws_ptr<uint16_t>(workspace, L.xs16 + (cfg->counter & 1u) * L.x16set));
  prep_only(p, parts);
  return launch_prep(prep_kernel(cfg->ragged != 0, rows_need_s16(cfg, bt, parts)), p, (hipStream_t)stream);
}

int dad_step_apply(const dad_config* cfg, const dad_state* st, void* workspace, void* stream_) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!st || !workspace) return DAD_E_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const DadWs L = dad_ws_layout(geom_of(cfg), max_splits_of(cfg), cfg->precision);
  float* normpart = ws_ptr<float>(workspace, L.normpart);
  const int nblk = (DAD_NPARAM + 1023) / 1024;
  int nnorm = DAD_REDUCE_BLOCKS;
  if (cfg->dp_world > 1) {
    hipLaunchKernelGGL(dad_norm, dim3(nblk), dim3(256), 0, stream, st->grad, normpart, 1.0f / (float)cfg->dp_world);
    DAD_TRY(hipGetLastError());
    nnorm = nblk;
  }
  DadOptimArgs oa;
  memset(&oa, 0, sizeof(oa));
  oa.cfg = *cfg;
  oa.student = st->student; oa.teacher = st->teacher; oa.exp_avg = st->exp_avg; oa.exp_avg_sq = st->exp_avg_sq;
  oa.grad = st->grad;
  oa.w1h_student = st->w1bf_student;
  oa.w1h_teacher = st->w1bf_teacher;
  oa.dacp = st->dacp; oa.tailf = st->tail; oa.normpart = normpart; oa.nnorm = nnorm;
  oa.losses_out = st->losses;
  tk_mark(TK_OPT0, stream);
  hipLaunchKernelGGL(dad_optim, dim3(nblk), dim3(DAD_OPTIM_THREADS), 0, stream, oa);
  DAD_TRY(hipGetLastError());
  tk_mark(TK_OPT1, stream);
  tk_end();
  return DAD_OK;
}

int dad_step_commit(const dad_config* cfg, const dad_state* st, void* workspace, void* stream_) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!st || !st->grad || !st->dacp || !st->tail || !workspace) return DAD_E_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (cfg->dp_world > 1) {
    const DadWs L = dad_ws_layout(geom_of(cfg), max_splits_of(cfg), cfg->precision);
    const int nblk = (DAD_NPARAM + 1023) / 1024;
    hipLaunchKernelGGL(dad_norm, dim3(nblk), dim3(256), 0, stream, st->grad, ws_ptr<float>(workspace, L.normpart),
                       1.0f / (float)cfg->dp_world);
    DAD_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(dad_commit_kernel, dim3(1), dim3(64), 0, stream, *cfg, st->grad, st->dacp, st->tail, st->losses);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

int dad_step(const dad_config* cfg, const dad_batch* batch, const dad_state* st, void* workspace, void* stream) {
  int rc = dad_step_compute(cfg, batch, st, workspace, stream);
  if (rc) return rc;
  return dad_step_apply(cfg, st, workspace, stream);
}

int dad_epoch_end(const dad_config* cfg, const dad_state* st, void* stream_) {
  if (!cfg || !st || !st->dacp) return DAD_E_ARG;
  hipLaunchKernelGGL(dad_epoch_end_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, st->dacp, cfg->dacp_beta,
                     cfg->dacp_one_m_beta);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

int dad_refresh_shadow(const dad_state* st, int precision, void* stream_) {
  if (!st || !st->student || !st->teacher || !st->w1bf_student || !st->w1bf_teacher) return DAD_E_ARG;
  if (precision != DAD_PREC_FP32 && !dad_prec16(precision)) return DAD_E_ARG;
  hipLaunchKernelGGL(dad_shadow_kernel, dim3((DAD_H * DAD_D + 255) / 256), dim3(256), 0, (hipStream_t)stream_,
                     st->student, st->teacher, st->w1bf_student, st->w1bf_teacher, precision == DAD_PREC_FP16 ? 1 : 0);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

}  // extern "C"
