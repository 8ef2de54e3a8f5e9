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

// the standalone preparation's kernel: the ragged sibling, the 16-bit-store sibling, or dad_prep
static void (*prep_kernel_of(const DadPrepArgs& p, bool ragged))(DadPrepArgs) {
  return ragged ? dad_prep_rg : dad_prep_s16_needed(p) ? dad_prep_s16 : dad_prep;
}

int launch_prep(const DadPrepArgs& p, hipStream_t stream, bool ragged) {
  int cus = 0;
  const int rc = device_cus(&cus);
  if (rc) return rc;
  hipLaunchKernelGGL(prep_kernel_of(p, ragged), dim3(prep_grid_of(cus)), dim3(DAD_PREP_THREADS), 0, stream, p);
  DAD_TRY(hipGetLastError());
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

// p restricted to `parts` (DAD_PREP_*) of its set
void prep_only(DadPrepArgs& p, int parts) {
  p.clean = (parts & DAD_PREP_CLEAN) ? 1 : 0;
  if (!(parts & DAD_PREP_NOISY)) p.warmup = 1;   // (dad_prep_rows: no noisy rows in a warm-up set)
}

// How each planned kernel (step_plan.h StepKernel) is launched: entry point and block size.
struct EncodeLaunch { void (*kernel)(DadEncodeArgs); int threads; };
const EncodeLaunch kEncodeLaunch[] = {   // [plan.encode - K_ENCODE_F32]
    {dad_encode_f32, DAD_ENC_F32_THREADS}, {dad_encode_wp, DAD_ENC_WS_THREADS}, {dad_encode_wp_f16, DAD_ENC_WS_THREADS}};
// (cp: the variants that also take the next batch's clean rows)
struct WgradLaunch {
  void (*kernel)(DadWgradArgs, DadReduceArgs);
  void (*cp)(DadWgradArgs, DadReduceArgs, DadPrepArgs);
  int threads;
};
const WgradLaunch kWgradLaunch[] = {   // [plan.wgrad - K_WGRAD_F32]
    {dad_wgrad_f32, nullptr, DAD_WGRAD_THREADS},
    {dad_wgrad_direct, nullptr, WGD_THREADS}, {nullptr, dad_wgrad_direct_cp, WGD_THREADS},
    {nullptr, dad_wgrad_direct_cps, WGD_THREADS},
    {dad_wgrad_direct_f16, nullptr, WGD_THREADS}, {nullptr, dad_wgrad_direct_f16_cp, WGD_THREADS},
    {nullptr, dad_wgrad_direct_f16_cps, WGD_THREADS}};
// the ragged step's siblings (dad_kernels.h `_rg`) of the 16-bit kernels above
const EncodeLaunch kEncodeLaunchRg[] = {   // [plan.encode - K_ENCODE_WP]
    {dad_encode_wp_rg, DAD_ENC_WS_THREADS}, {dad_encode_wp_f16_rg, DAD_ENC_WS_THREADS}};
const WgradLaunch kWgradLaunchRg[2] = {    // [fp16]: plain, and with the (ragged, store) next batch's clean rows
    {dad_wgrad_direct_rg, dad_wgrad_direct_cps_rg, WGD_THREADS}, {dad_wgrad_direct_f16_rg, dad_wgrad_direct_f16_cps_rg, WGD_THREADS}};
struct ReduceLaunch { void (*kernel)(DadReduceArgs); int threads; };
const ReduceLaunch kReduceLaunch[] = {{dad_reduce, DAD_REDUCE_THREADS}, {dad_reduce_w, 64}};   // [plan.reduce - K_REDUCE]

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
  const int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cus < 2 || !out || (defer & ~(DAD_PREP_CLEAN | DAD_PREP_NOISY)) != 0) return DAD_E_ARG;
  const int nrc = check_next_batch(next_cfg, next_batch);
  if (nrc) return nrc;
  const StepPlan p = plan_step(cfg, next_cfg, next_batch, defer, cus);
  if (p.encode_rc) return p.encode_rc;
  *out = dad_step_plan_info{p.splits, p.max_splits, p.prep_grid, p.encode_grid, p.ws_nt, p.ws_ns, p.pool_grid,
                            p.tail_grid, p.tail_prep, p.tail_prep == DAD_PREP_CLEAN, p.wgrad_grid, p.wgrad_clean,
                            p.wgrad_store, p.reduce_grid, p.prepped, p.pending, kStepKernelName[p.encode],
                            kStepKernelName[p.tail], kStepKernelName[p.wgrad], kStepKernelName[p.reduce]};
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
  *bytes = dad_ws_layout(geom_of(cfg), max_splits_of(cfg), cfg->precision).bytes;
  return DAD_OK;
}

}  // extern "C"

// The launches of one step: validate, plan (step_plan.h), fill the argument blocks, launch what the
// plan says.  (ncfg, nbt, defer): dad_step_backward_ahead_split's next batch and deferred parts.
static int step_compute_phases(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                               void* stream_, bool do_encode, bool do_backward, const dad_config* ncfg = nullptr,
                               const dad_batch* nbt = nullptr, int* prepped = nullptr, int defer = 0,
                               int* pending = nullptr) {
  if (prepped) *prepped = 0;
  if (pending) *pending = 0;
  int rc = check_step_args(cfg, bt, st, workspace);
  if (rc) return rc;
  rc = check_next_batch(ncfg, nbt);
  if (rc) return rc;
  int cus = 0;
  rc = device_cus(&cus);
  if (rc) return rc;
  const StepPlan plan = plan_step(cfg, ncfg, nbt, defer, cus);

  const bool explicit_rng = cfg->rng_mode == DAD_RNG_EXPLICIT;
  const DadStoreRows src = store_rows_of(bt);
  hipStream_t stream = (hipStream_t)stream_;
  const DadGeom G = geom_of(cfg);
  const DadWs L = dad_ws_layout(G, plan.max_splits, cfg->precision);
  const Keys k = keys_of(cfg);
  float* part_sum = ws_ptr<float>(workspace, L.part_sum);
  float* part_cnt = ws_ptr<float>(workspace, L.part_cnt);
  uint32_t* bits = ws_ptr<uint32_t>(workspace, L.bits);
  float* vlen = ws_ptr<float>(workspace, L.vlen);
  float* cnt_tot = ws_ptr<float>(workspace, L.cnt_tot);
  float* ge = ws_ptr<float>(workspace, L.ge);
  float* ge_ecda = ws_ptr<float>(workspace, L.ge_ecda);
  float* normpart = ws_ptr<float>(workspace, L.normpart);
  float* ecda_scratch = ws_ptr<float>(workspace, L.ecda);
  float* gzb = ws_ptr<float>(workspace, L.gzb);
  uint32_t* eflag = ws_ptr<uint32_t>(workspace, L.eflag);
  uint32_t* pool_ready = ws_ptr<uint32_t>(workspace, L.ready);
  // 16-bit modes: this step's prepared set (parity of the step counter; the next step's set is
  // the other one, so preparing it in this step's launches leaves this one intact for wgrad)
  uint16_t* xs16 = ws_ptr<uint16_t>(workspace, L.xs16 + (cfg->counter & 1u) * L.x16set);
  const size_t nrc = (size_t)G.Bc * G.Tc, nrn = (size_t)G.Bn * G.Tn;

  // 1. fused augmentation + encoder GEMMs + pooling partials
  if (do_encode) {
    if (plan.encode_rc) return plan.encode_rc;
    DadEncodeArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.g = G; ea.warmup = cfg->warmup;
    ea.mask_len = cfg->mask_len; ea.start_hi = cfg->start_hi;
    // (the FP32 encoder reads the rows, f32 by check_batch_dtypes; the 16-bit ones read the prepared set)
    ea.xc = static_cast<const float*>(bt->xc); ea.mc = bt->mc; ea.xn = static_cast<const float*>(bt->xn); ea.mn = bt->mn;
    ea.src = src;
    ea.w1_student = st->student + DAD_OFF_W1; ea.b1_student = st->student + DAD_OFF_B1;
    ea.w1_teacher = st->teacher + DAD_OFF_W1; ea.b1_teacher = st->teacher + DAD_OFF_B1;
    ea.w1h_student = st->w1bf_student;
    ea.w1h_teacher = st->w1bf_teacher;
    ea.pool_ready = pool_ready;
    if (explicit_rng) { ea.nw = bt->nw; ea.ns = bt->ns; ea.u = bt->u; ea.start = bt->start; }
    ea.key_weak = k.weak; ea.key_strong = k.strong; ea.key_feat = k.feat; ea.key_tstart = k.tstart;
    ea.weak_std = cfg->weak_std; ea.strong_std = cfg->strong_std; ea.feat_p = cfg->feat_p;
    ea.part_sum = part_sum; ea.part_cnt = part_cnt; ea.bits = bits;
    ea.ws_nt = plan.ws_nt; ea.ws_ns = plan.ws_ns;
    ea.x16c = xs16; ea.x16s = xs16 + nrc * DAD_D; ea.x16w = ea.x16s + (cfg->warmup ? 0 : nrn) * DAD_D;
    tk_begin();
    tk_mark(TK_E0, stream);
    if (plan.prep_grid) {
      const DadPrepArgs own = prep_args(cfg, bt, xs16);
      hipLaunchKernelGGL(prep_kernel_of(own, cfg->ragged != 0), dim3(plan.prep_grid), dim3(DAD_PREP_THREADS), 0, stream,
                         own);
      DAD_TRY(hipGetLastError());
    }
    const EncodeLaunch& enc = cfg->ragged ? kEncodeLaunchRg[plan.encode - K_ENCODE_WP] : kEncodeLaunch[plan.encode - K_ENCODE_F32];
    hipLaunchKernelGGL(enc.kernel, dim3(plan.encode_grid), dim3(enc.threads), 0, stream, ea);
    DAD_TRY(hipGetLastError());
    tk_mark(TK_E1, stream);
  }
  if (!do_backward) return DAD_OK;
  if (prepped) *prepped = plan.prepped;
  if (pending) *pending = plan.pending;

  // 2. pooled embeddings + classifier logits: a launch of its own, or the spare blocks of the
  //    wave-centric tail launch (no pool timing point then: that launch is timed from the encoder's end)
  DadPoolArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.g = G; pa.warmup = cfg->warmup;
  pa.mc = bt->mc; pa.mn = bt->mn; pa.part_sum = part_sum;
  pa.student = st->student; pa.teacher = st->teacher;
  if (explicit_rng) { pa.keep1 = bt->keep1; pa.keep2 = bt->keep2; }
  pa.key_drop1 = k.drop1; pa.key_drop2 = k.drop2;
  pa.p_drop = cfg->p_drop; pa.drop_scale = cfg->drop_scale;
  pa.emb = st->emb; pa.vlen = vlen; pa.logits = st->logits;
  pa.part_cnt = part_cnt; pa.cnt_tot = cnt_tot;
  pa.eflag = eflag; pa.tail_terms = st->tail + DAD_T_ECDA_TERM;
  pa.range_flag = reinterpret_cast<uint32_t*>(st->tail + DAD_T_RANGE);
  if (cfg->ragged) { pa.lenc = bt->lenc; pa.lenn = bt->lenn; }
  if (plan.pool_grid) {
    hipLaunchKernelGGL(cfg->ragged ? dad_pool_rg : dad_pool, dim3(plan.pool_grid), dim3(DAD_POOL_THREADS), 0, stream, pa);
    DAD_TRY(hipGetLastError());
    tk_mark(TK_POOL, stream);
  } else {
    pa.ready = pool_ready;   // (zeroed by this step's encoder)
  }

  // 3. losses, DACP mask, analytic backward to dL/de and the classifier grads
  DadTailArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.cfg = *cfg; ta.yc = bt->yc; ta.logits = st->logits; ta.emb = st->emb; ta.student = st->student;
  if (explicit_rng) { ta.keep1 = bt->keep1; ta.keep2 = bt->keep2; }
  ta.key_drop1 = k.drop1; ta.key_drop2 = k.drop2;
  ta.dacp = st->dacp; ta.tailf = st->tail; ta.ge = ge; ta.ge_ecda = ge_ecda; ta.grad = st->grad;
  ta.gzb = gzb; ta.eflag = eflag;
  // 4. ECDA (class-aware MMD + compactness + repulsion) and its embedding grads: after the
  //    warm-up, in the same launch as the tail (block 0 = tail, blocks 1..C = classes)
  DadEcdaArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.cfg = *cfg; ca.yc = bt->yc; ca.emb = st->emb; ca.tailf = st->tail;
  ca.tail_terms = st->tail + DAD_T_ECDA_TERM; ca.ge = ge_ecda; ca.scratch = ecda_scratch; ca.eflag = eflag;
  ca.sink = ws_ptr<float>(workspace, L.gflat);
  // the next batch's rows this step prepares: pp in the tail launch, pcw (its clean rows) in the
  // weight-gradient launch; x16 = NULL: nothing
  DadPrepArgs pp, pcw;
  memset(&pp, 0, sizeof(pp));
  memset(&pcw, 0, sizeof(pcw));
  if (plan.prepped) {
    const DadPrepArgs next = prep_args(ncfg, nbt, ws_ptr<uint16_t>(workspace, L.xs16 + (ncfg->counter & 1u) * L.x16set));
    if (plan.wgrad_clean) pcw = next;
    if (plan.tail_prep) { pp = next; prep_only(pp, plan.tail_prep); }
  }
  const dim3 tgrid(plan.tail_grid), tblock(DAD_TAIL_THREADS);
  switch (plan.tail) {
    case K_TAIL: hipLaunchKernelGGL(dad_tail, tgrid, tblock, 0, stream, ta); break;
    case K_TAIL_ECDA: hipLaunchKernelGGL(dad_tail_ecda, tgrid, tblock, 0, stream, ta, ca); break;
    default:   // (the `_s16` sibling when the rows it prepares lie in a 16-bit store, dad_kernels.h)
      //  a ragged step: its `_rg` sibling, whose pooling sums live slabs only)
      hipLaunchKernelGGL(cfg->ragged ? dad_tail_ecda_w_rg
                                     : pp.x16 && dad_prep_s16_needed(pp) ? dad_tail_ecda_w_s16 : dad_tail_ecda_w,
                         tgrid, tblock, 0, stream, ta, ca, pp, pa);
      break;
  }
  DAD_TRY(hipGetLastError());
  tk_mark(TK_TAIL, stream);

  // 5. dW1 as one direct split-K GEMM (G = ReLU' * dL/de / len rebuilt from the tail's dL/dz
  //    and the ECDA rows), then the split sums with db1, dW2, loss totals, squared-norm partials
  DadWgradArgs wa;
  memset(&wa, 0, sizeof(wa));
  wa.g = G; wa.warmup = cfg->warmup;
  wa.mask_len = cfg->mask_len; wa.start_hi = cfg->start_hi;
  wa.xc = static_cast<const float*>(bt->xc); wa.xn = static_cast<const float*>(bt->xn); wa.src = src;   // (FP32 only)
  if (explicit_rng) { wa.ns = bt->ns; wa.u = bt->u; wa.start = bt->start; }
  wa.key_strong = k.strong; wa.key_feat = k.feat; wa.key_tstart = k.tstart;
  wa.strong_std = cfg->strong_std; wa.feat_p = cfg->feat_p;
  wa.bits = bits; wa.ge = ge; wa.vlen = vlen; wa.xs16 = xs16;
  wa.splits = plan.splits; wa.ntiles = plan.wgrad_tiles;
  wa.wpart = ws_ptr<float>(workspace, L.wpart);
  DadReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.g = G; ra.warmup = cfg->warmup;
  ra.want_norm = cfg->dp_world == 1;
  ra.w_kl = cfg->w_kl; ra.w_ecda = cfg->w_ecda;
  ra.ge_ecda = ge_ecda;
  ra.gzb = gzb; ra.eflag = eflag; ra.student = st->student; ra.emb = st->emb;
  if (explicit_rng) { ra.keep1 = bt->keep1; ra.keep2 = bt->keep2; }
  ra.key_drop1 = k.drop1; ra.key_drop2 = k.drop2; ra.p_drop = cfg->p_drop; ra.drop_scale = cfg->drop_scale;
  ra.ge = ge; ra.vlen = vlen; ra.cnt_tot = cnt_tot; ra.tailf = st->tail;
  ra.grad = st->grad; ra.normpart = normpart;
  ra.pool_abort = plan.pool_grid ? nullptr : pool_ready + DAD_POOL_ABORT;
  ra.splits = plan.splits; ra.wpart = wa.wpart;
  const WgradLaunch& wg = kWgradLaunch[plan.wgrad - K_WGRAD_F32];
  if (cfg->ragged) {
    const WgradLaunch& rg = kWgradLaunchRg[cfg->precision == DAD_PREC_FP16];
    if (plan.wgrad_clean) hipLaunchKernelGGL(rg.cp, dim3(plan.wgrad_grid), dim3(rg.threads), 0, stream, wa, ra, pcw);
    else hipLaunchKernelGGL(rg.kernel, dim3(plan.wgrad_grid), dim3(rg.threads), 0, stream, wa, ra);
  } else if (wg.cp) {
    auto cp = wg.cp;
    if (plan.wgrad_store && pcw.xc_type() != DAD_STORE_F32)
      cp = cfg->precision == DAD_PREC_FP16 ? dad_wgrad_direct_f16_cps_s16 : dad_wgrad_direct_cps_s16;
    hipLaunchKernelGGL(cp, dim3(plan.wgrad_grid), dim3(wg.threads), 0, stream, wa, ra, pcw);
  }
  else hipLaunchKernelGGL(wg.kernel, dim3(plan.wgrad_grid), dim3(wg.threads), 0, stream, wa, ra);
  DAD_TRY(hipGetLastError());
  tk_mark(TK_WGRAD, stream);
  const ReduceLaunch& red = kReduceLaunch[plan.reduce - K_REDUCE];
  hipLaunchKernelGGL(red.kernel, dim3(plan.reduce_grid), dim3(red.threads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
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
  return step_compute_phases(cfg, bt, st, workspace, stream, false, true, next_cfg, next_batch, prepped);
}

int dad_step_backward_ahead_split(const dad_config* cfg, const dad_batch* bt, const dad_state* st, void* workspace,
                                  void* stream, const dad_config* next_cfg, const dad_batch* next_batch, int defer,
                                  int* prepped, int* pending) {
  if (!pending || (defer & ~(DAD_PREP_CLEAN | DAD_PREP_NOISY)) != 0) return DAD_E_ARG;
  return step_compute_phases(cfg, bt, st, workspace, stream, false, true, next_cfg, next_batch, prepped, defer,
                             pending);
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
  return launch_prep(p, (hipStream_t)stream, cfg->ragged != 0);
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
