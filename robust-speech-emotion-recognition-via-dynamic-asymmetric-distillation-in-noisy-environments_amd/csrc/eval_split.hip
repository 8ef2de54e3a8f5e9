// Whole-split evaluation, store-fed: one call runs the eval-mode forward of the student (and,
// on the same row reads, the teacher) over EVERY utterance of a FeatureStore split and leaves
// what validation and anchor calibration report in one small result block.
//
// Replaces, per split (not per batch):
//   Trainer.validate                 I/train.py:522-564  (predictions -> confusion matrix; the
//                                    teacher pass of the disagreement rate)
//   Trainer._run_anchor_calibration  I/train.py:317-357  (per-class mean / std of the certainty score)
//   SSRLModel.get_embeddings         I/model.py:247-265  (split-wide)
//
// Three launches, no host work in between:
//   dad_eval_encode   one wave = one 32-frame slab of one utterance x all 256 hidden units (the work
//                     unit of dad_encode_f32).  Jobs exist only for valid frames: utterance i owns slabs
//                     [slab_off[i], slab_off[i+1]), slab_off[i+1] - slab_off[i] = ceil(len_i / 32).
//                     Frame t is store row rows[i] + t, read in place (f32 / f16 / bf16, widened
//                     exactly); past the last frame the row is clamped and the epilogue masks it.
//                     With a teacher, each row read feeds both networks' GEMMs.  Epilogue: bias, ReLU,
//                     sum over the slab's valid rows -> part[slab][256] per network.
//   dad_eval_head     one wave per utterance: slab partials summed in slab order, / max(len, 1),
//                     classifier, softmax, certainty score, first-maximum argmax (dad_predict_head's
//                     arithmetic), student and teacher.
//   dad_eval_result   one workgroup: confusion matrices, disagreement / skipped / non-finite counts
//                     (integer LDS atomics) and the per-class float64 two-pass score moments (strided
//                     per-thread sums and a fixed LDS tree: no floating-point atomics, so two calls
//                     on the same inputs give the same bits).
// FP32: v_mfma_f32_32x32x2_f32, the k order and epilogue order of dad_encode_f32, so embeddings equal
// the per-batch path's bit for bit.  FP16: rows and a row-major fp16 copy of W1 (made inside the
// call: the weights change every epoch) on v_mfma_f32_32x32x16_f16, fp32 accumulation.
#include <cstring>

#include "dad_common.h"
#include "dad_kernels.h"
#include "eval_rows.h"   // row loaders, the slab GEMM loop and epilogue, the head arithmetic (shared with eval_windows.hip)

namespace {

constexpr int kEncThreads = 256;     // 4 waves, one slab each
constexpr int kHeadWaves = 4;
constexpr int kResThreads = 256;

struct EvalEncArgs {
  const void* store;
  const int64_t* rows; const int32_t* lens; const int32_t* slab_off;
  int n, slabs;
  const float* student; const float* teacher;        // flat [W1|b1|W2|b2]
  const uint16_t* w1h_s; const uint16_t* w1h_t;      // FP16: row-major fp16 W1 copies
  float* part_s; float* part_t;                      // [slabs][256]
};

struct EvalHeadArgs {
  int n, slabs, use_entropy;
  const int32_t* lens; const int32_t* slab_off;
  const float* part_s; const float* part_t;
  const float* student; const float* teacher;
  float* emb; float* logits; float* probs; float* score; int64_t* pred;
  float* t_emb; float* t_logits; int64_t* t_pred;
  int32_t* ws_pred_s; int32_t* ws_pred_t; float* ws_score; int32_t* ws_bad;
};

struct EvalResArgs {
  int n, with_teacher;
  const int64_t* labels;
  const int32_t* pred_s; const int32_t* pred_t; const float* score; const int32_t* bad;
  int64_t* counts; double* moments;
};

template <int DT, bool TEACH, bool F16>
__global__ __launch_bounds__(kEncThreads) void dad_eval_encode(EvalEncArgs a) {
  DAD_GUARD_BLOCK(kEncThreads);
  const int lane = threadIdx.x & 63;
  const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kEncThreads / 64) + (threadIdx.x >> 6)));
  if (job >= a.slabs) return;
  const int u = slab_owner(a.slab_off, a.n, job);
  const int len = a.lens[u];
  const int c = job - a.slab_off[u];
  const int i = lane & 31, kh = lane >> 5;
  const int t = c * DAD_SLAB + i;
  const uint32_t vbits = (uint32_t)__ballot(t < len && c >= 0);
  f32x16 acc0[DAD_HT], acc1[DAD_HT];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    acc0[ht] = f32x16{};
    acc1[ht] = f32x16{};
  }
  if (vbits != 0u) {   // a table that disagrees with lens reads nothing and writes zeros
    // past the last frame: the utterance's last row again (masked by vbits in the epilogue)
    const size_t row = (size_t)(a.rows[u] + (int64_t)min(t, len - 1));
    if constexpr (F16) {
      const uint16_t* Ws = a.w1h_s + (size_t)i * DAD_D + 8 * kh;
      const uint16_t* Wt = TEACH ? a.w1h_t + (size_t)i * DAD_D + 8 * kh : nullptr;
      eval_slab_f16<DT, TEACH>(a.store, row * DAD_D + 8 * kh, Ws, Wt, acc0, acc1);
    } else {
      const float* Ws = a.student + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh;
      const float* Wt = TEACH ? a.teacher + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh : nullptr;
      eval_slab_f32<DT, TEACH>(a.store, row * DAD_D + 4 * kh, Ws, Wt, acc0, acc1);
    }
  }
  eval_epilogue(acc0, a.student + DAD_OFF_B1, a.part_s + (size_t)job * DAD_H, vbits);
  if constexpr (TEACH) eval_epilogue(acc1, a.teacher + DAD_OFF_B1, a.part_t + (size_t)job * DAD_H, vbits);
}

// row-major fp16 copies of both networks' W1 (blockIdx.y: 0 student, 1 teacher)
__global__ __launch_bounds__(256) void dad_eval_w1h(const float* student, const float* teacher, uint16_t* ws,
                                                    uint16_t* wt) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)DAD_H * DAD_D) return;
  if (blockIdx.y == 0) ws[i] = dad_half_bits(student[DAD_OFF_W1 + i], true);
  else wt[i] = dad_half_bits(teacher[DAD_OFF_W1 + i], true);
}

// One network's head for utterance u: its slab partials summed in slab order, then eval_head_pooled.
__device__ __forceinline__ int eval_head_one(const float* part, int s0, int s1, float len, const float* flat,
                                             int use_entropy, size_t u, float* emb, float* logits, float* probs,
                                             float* score_out, float* score_ws, bool* bad) {
  const int lane = threadIdx.x & 63;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = s0; c < s1; ++c) s += *reinterpret_cast<const f32x4*>(part + (size_t)c * DAD_H + 4 * lane);
  return eval_head_pooled(s, len, flat, use_entropy, u, emb, logits, probs, score_out, score_ws, bad);
}

__global__ __launch_bounds__(64 * kHeadWaves) void dad_eval_head(EvalHeadArgs a) {
  DAD_GUARD_BLOCK(64 * kHeadWaves);
  const int lane = threadIdx.x & 63;
  const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kHeadWaves + (threadIdx.x >> 6)));
  if (u >= a.n) return;
  const int len = max(a.lens[u], 0);
  int s0 = a.slab_off[u], s1 = a.slab_off[u + 1];
  if (s0 < 0 || s1 > a.slabs || s1 - s0 != (len + DAD_SLAB - 1) / DAD_SLAB) s0 = s1 = 0;   // inconsistent table: a zero embedding
  bool bad_s = false, bad_t = false;
  const int ps = eval_head_one(a.part_s, s0, s1, (float)len, a.student, a.use_entropy, (size_t)u, a.emb, a.logits,
                               a.probs, a.score, a.ws_score, &bad_s);
  int pt = ps;
  if (a.teacher)
    pt = eval_head_one(a.part_t, s0, s1, (float)len, a.teacher, a.use_entropy, (size_t)u, a.t_emb, a.t_logits,
                       nullptr, nullptr, nullptr, &bad_t);
  if (lane == 0) {
    if (a.pred) a.pred[u] = ps;
    if (a.teacher && a.t_pred) a.t_pred[u] = pt;
    a.ws_pred_s[u] = ps;
    a.ws_pred_t[u] = pt;
    a.ws_bad[u] = (bad_s || bad_t) ? 1 : 0;
  }
}

// fixed-order sum of one double per thread over the workgroup (result in every thread)
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kResThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kResThreads) void dad_eval_result(EvalResArgs a) {
  DAD_GUARD_BLOCK(kResThreads);
  __shared__ unsigned int cnt[DAD_EV_COUNTS];
  __shared__ double red[kResThreads];
  const int tid = threadIdx.x;
  if (tid < DAD_EV_COUNTS) cnt[tid] = 0u;
  __syncthreads();
  for (int u = tid; u < a.n; u += kResThreads) {
    const long y = a.labels ? (long)a.labels[u] : -1;
    const int ps = a.pred_s[u], pt = a.pred_t[u];
    if (y >= 0 && y < DAD_C) {
      atomicAdd(&cnt[DAD_EV_CONF_STUDENT + (int)y * DAD_C + ps], 1u);
      if (a.with_teacher) atomicAdd(&cnt[DAD_EV_CONF_TEACHER + (int)y * DAD_C + pt], 1u);
      atomicAdd(&cnt[DAD_EV_N_LABELLED], 1u);
    } else {
      atomicAdd(&cnt[DAD_EV_N_SKIPPED], 1u);
    }
    if (a.with_teacher && ps != pt) atomicAdd(&cnt[DAD_EV_DISAGREE], 1u);
    if (a.bad[u]) atomicAdd(&cnt[DAD_EV_N_NONFINITE], 1u);
  }
  __syncthreads();
  if (tid < DAD_EV_COUNTS) a.counts[tid] = tid == DAD_EV_N ? (int64_t)a.n : (int64_t)cnt[tid];
  // per true class: count, mean, population variance of the student's score, float64, two passes
  for (int c = 0; c < DAD_C; ++c) {
    unsigned int k = 0;
    for (int p = 0; p < DAD_C; ++p) k += cnt[DAD_EV_CONF_STUDENT + c * DAD_C + p];
    double s = 0.0;
    for (int u = tid; u < a.n; u += kResThreads)
      if (a.labels && a.labels[u] == c) s += (double)a.score[u];
    const double tot = block_sum_d(s, red);
    const double mean = k ? tot / (double)k : 0.0;
    double q = 0.0;
    for (int u = tid; u < a.n; u += kResThreads)
      if (a.labels && a.labels[u] == c) {
        const double dlt = (double)a.score[u] - mean;
        q += dlt * dlt;
      }
    const double sq = block_sum_d(q, red);
    if (tid == 0) {
      a.moments[c * DAD_EV_MOMENTS + DAD_EV_M_COUNT] = (double)k;
      a.moments[c * DAD_EV_MOMENTS + DAD_EV_M_MEAN] = mean;
      a.moments[c * DAD_EV_MOMENTS + DAD_EV_M_VAR] = k ? sq / (double)k : 0.0;
    }
  }
}

struct EvalWs {
  size_t part_s, part_t, pred_s, pred_t, score, bad, w1h_s, w1h_t, bytes;
};

EvalWs eval_ws_layout(int64_t n, int64_t slabs, int precision, int with_teacher) {
  EvalWs w;
  size_t off = 0;
  const size_t sl = (size_t)(slabs > 0 ? slabs : 1);
  w.part_s = off; off = dad_align(off + sizeof(float) * sl * DAD_H);
  w.part_t = off; off = dad_align(off + (with_teacher ? sizeof(float) * sl * DAD_H : 0));
  w.pred_s = off; off = dad_align(off + sizeof(int32_t) * (size_t)n);
  w.pred_t = off; off = dad_align(off + sizeof(int32_t) * (size_t)n);
  w.score = off;  off = dad_align(off + sizeof(float) * (size_t)n);
  w.bad = off;    off = dad_align(off + sizeof(int32_t) * (size_t)n);
  const size_t wb = precision == DAD_PREC_FP16 ? sizeof(uint16_t) * DAD_H * DAD_D : 0;
  w.w1h_s = off;  off = dad_align(off + wb);
  w.w1h_t = off;  off = dad_align(off + (with_teacher ? wb : 0));
  w.bytes = off;
  return w;
}

bool eval_shape_ok(int64_t n, int64_t slabs) {
  // every utterance holds at most 2^31 / 32 slabs, and the kernels index slabs with 32 bits
  return n >= 1 && n <= 0x7fffffffLL && slabs >= 0 && slabs <= 0x7fffffffLL && slabs <= n * (int64_t)(1 << 26);
}

template <int DT>
void launch_encode(const EvalEncArgs& ea, bool teach, bool f16, hipStream_t stream) {
  const dim3 grid((unsigned)((ea.slabs + kEncThreads / 64 - 1) / (kEncThreads / 64))), block(kEncThreads);
  if (f16) {
    if (teach) hipLaunchKernelGGL((dad_eval_encode<DT, true, true>), grid, block, 0, stream, ea);
    else hipLaunchKernelGGL((dad_eval_encode<DT, false, true>), grid, block, 0, stream, ea);
  } else {
    if (teach) hipLaunchKernelGGL((dad_eval_encode<DT, true, false>), grid, block, 0, stream, ea);
    else hipLaunchKernelGGL((dad_eval_encode<DT, false, false>), grid, block, 0, stream, ea);
  }
}

}  // namespace

extern "C" size_t dad_eval_workspace_bytes(int64_t n, int64_t slabs, int precision, int with_teacher) {
  if (!eval_shape_ok(n, slabs)) return 0;
  return eval_ws_layout(n, slabs, precision, with_teacher ? 1 : 0).bytes;
}

extern "C" int dad_eval_split(const dad_eval_args* args, void* workspace, void* stream_) {
  if (!args || !workspace) return DAD_E_ARG;
  if (!args->store || !args->rows || !args->lens || !args->slab_off || !args->student || !args->counts ||
      !args->moments)
    return DAD_E_ARG;
  const int dt = args->store_dtype;
  if (dt != DAD_STORE_F32 && dt != DAD_STORE_F16 && dt != DAD_STORE_BF16) return DAD_E_ARG;
  if (args->precision == DAD_PREC_BF16) return DAD_E_UNSUPPORTED;
  if (args->precision != DAD_PREC_FP32 && args->precision != DAD_PREC_FP16) return DAD_E_ARG;
  if (!eval_shape_ok(args->n, args->slabs)) return DAD_E_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const bool teach = args->teacher != nullptr, f16 = args->precision == DAD_PREC_FP16;
  const EvalWs L = eval_ws_layout(args->n, args->slabs, args->precision, teach ? 1 : 0);
  char* ws = (char*)workspace;

  EvalEncArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.store = args->store; ea.rows = args->rows; ea.lens = args->lens; ea.slab_off = args->slab_off;
  ea.n = (int)args->n; ea.slabs = (int)args->slabs;
  ea.student = args->student; ea.teacher = args->teacher;
  ea.w1h_s = (const uint16_t*)(ws + L.w1h_s); ea.w1h_t = (const uint16_t*)(ws + L.w1h_t);
  ea.part_s = (float*)(ws + L.part_s); ea.part_t = (float*)(ws + L.part_t);
  if (ea.slabs > 0) {
    if (f16) {
      hipLaunchKernelGGL(dad_eval_w1h, dim3((DAD_H * DAD_D + 255) / 256, teach ? 2 : 1), dim3(256), 0, stream,
                         args->student, args->teacher, (uint16_t*)(ws + L.w1h_s), (uint16_t*)(ws + L.w1h_t));
      DAD_TRY(hipGetLastError());
    }
    switch (dt) {
      case DAD_STORE_F16: launch_encode<DAD_STORE_F16>(ea, teach, f16, stream); break;
      case DAD_STORE_BF16: launch_encode<DAD_STORE_BF16>(ea, teach, f16, stream); break;
      default: launch_encode<DAD_STORE_F32>(ea, teach, f16, stream); break;
    }
    DAD_TRY(hipGetLastError());
  }

  EvalHeadArgs ha;
  memset(&ha, 0, sizeof(ha));
  ha.n = ea.n; ha.slabs = ea.slabs; ha.use_entropy = args->use_entropy;
  ha.lens = args->lens; ha.slab_off = args->slab_off;
  ha.part_s = ea.part_s; ha.part_t = ea.part_t;
  ha.student = args->student; ha.teacher = args->teacher;
  ha.emb = args->emb; ha.logits = args->logits; ha.probs = args->probs; ha.score = args->score; ha.pred = args->pred;
  ha.t_emb = args->t_emb; ha.t_logits = args->t_logits; ha.t_pred = args->t_pred;
  ha.ws_pred_s = (int32_t*)(ws + L.pred_s); ha.ws_pred_t = (int32_t*)(ws + L.pred_t);
  ha.ws_score = (float*)(ws + L.score); ha.ws_bad = (int32_t*)(ws + L.bad);
  hipLaunchKernelGGL(dad_eval_head, dim3((unsigned)((ea.n + kHeadWaves - 1) / kHeadWaves)), dim3(64 * kHeadWaves), 0,
                     stream, ha);
  DAD_TRY(hipGetLastError());

  EvalResArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.n = ea.n; ra.with_teacher = teach ? 1 : 0; ra.labels = args->labels;
  ra.pred_s = ha.ws_pred_s; ra.pred_t = ha.ws_pred_t; ra.score = ha.ws_score; ra.bad = ha.ws_bad;
  ra.counts = args->counts; ra.moments = args->moments;
  hipLaunchKernelGGL(dad_eval_result, dim3(1), dim3(kResThreads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}
