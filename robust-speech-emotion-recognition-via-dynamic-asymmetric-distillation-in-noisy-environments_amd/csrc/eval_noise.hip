// Noise response of a split, store-fed: one call evaluates every utterance of a FeatureStore split at K levels of
// additive Gaussian noise x_t + sigma_k n_t of ONE draw, in one pass over the store (dad.h, "noise response of a
// split").
//
// The encoder is frame-wise and linear before its ReLU, W1 (x_t + s n_t) + b1 = W1 x_t + s W1 n_t + b1, so the
// slab kernel keeps two accumulators on one W1 fragment, acc0 = x W1 and acc1 = n W1 (the 256 accumulator
// registers of dad_eval_encode's teacher instance), and a level costs an epilogue and a head.
//
// Three launches (plus the fp16 copy of W1 in FP16), no host work in between:
//   dad_noise_encode   dad_eval_encode's work unit (one wave = one 32-frame slab x all 256 hidden units, rows read
//                      in place).  The noise A fragment is generated in registers by the counter RNG (noise_key /
//                      noise_pair of eval_rows.h: a pure function of seed, draw, utterance, frame, channel) or, in
//                      explicit mode, loaded from the slab-aligned array; both in the MFMA's lane layout.  Epilogue
//                      per level: relu(fma(sigma_k, acc1, acc0) + b1) summed over the slab's valid rows
//                      -> part[slab][k][256].
//   dad_noise_head     one wave per utterance walks its levels in order: slab partials summed in slab order,
//                      eval_head_pooled's arithmetic, and against level 0's embedding and log-softmax the drift,
//                      the KL term and the break level.
//   dad_noise_result   one workgroup: the DAD_EN_* block (integer LDS atomics; float64 sums by strided per-thread
//                      sums and a fixed LDS tree).
// No floating-point atomics anywhere.  A level with sigma = 0 repeats dad_eval_split's arithmetic exactly:
// fma(0, acc1, acc0) = acc0 for a finite acc1, and the k order, epilogue order and head are the same code.
#include <cmath>
#include <cstring>

#include "dad_common.h"
#include "dad_kernels.h"
#include "eval_rows.h"

namespace {

constexpr int kEncThreads = 256;     // 4 waves, one slab each
constexpr int kHeadWaves = 4;
constexpr int kResThreads = 256;
constexpr int kDrawThreads = DAD_D / 4;   // one frame's 192 channel quads
static_assert(DAD_EN_COUNTS <= kResThreads && DAD_EN_SUMS <= kResThreads, "dad_noise_result's thread roles");

struct NoiseEncArgs {
  const void* store;
  const int64_t* rows; const int32_t* lens; const int32_t* slab_off;
  int n, slabs, levels;
  const float* params;               // flat [W1|b1|W2|b2]
  const uint16_t* w1h;               // FP16: row-major fp16 W1 copy
  const float* noise;                // explicit mode
  uint32_t skey;                     // counter mode: the stream key
  float sigma[DAD_EN_MAX_LEVELS];
  float* part;                       // [slabs][levels][256]
};

struct NoiseHeadArgs {
  int n, slabs, levels, use_entropy;
  const int32_t* lens; const int32_t* slab_off;
  const float* part; const float* params;
  float* emb; float* logits; float* probs; float* score; int64_t* pred; float* drift; float* kl; int32_t* break_level;
  int32_t* ws_pred; float* ws_score; float* ws_drift; float* ws_kl; int32_t* ws_bad; int32_t* ws_break;
};

struct NoiseResArgs {
  int n, levels;
  const int64_t* labels;
  const int32_t* ws_pred; const float* ws_score; const float* ws_drift; const float* ws_kl;
  const int32_t* ws_bad; const int32_t* ws_break;
  int64_t* counts; double* sums;
};

struct NoiseDrawArgs {
  const int32_t* lens; const int32_t* slab_off;
  int n, slabs;
  uint32_t skey;
  float* out;                        // [32 * slabs][768]
};

template <int DT, bool F16, bool EXPL>
__global__ __launch_bounds__(kEncThreads) void dad_noise_encode(NoiseEncArgs a) {
  DAD_GUARD_BLOCK(kEncThreads);
  const int lane = threadIdx.x & 63;
  const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kEncThreads / 64) + (threadIdx.x >> 6)));
  if (job >= a.slabs) return;
  const int u = slab_owner(a.slab_off, a.n, job);
  const int len = a.lens[u];
  const int s0 = a.slab_off[u];
  const int c = job - s0;
  const int i = lane & 31, kh = lane >> 5;
  const int t = c * DAD_SLAB + i;
  const uint32_t vbits = (uint32_t)__ballot(t < len && c >= 0);
  float* part = a.part + (size_t)job * a.levels * DAD_H;
  if (vbits == 0u) {                 // a table that disagrees with lens reads nothing and writes zeros
    for (int e = lane; e < a.levels * DAD_H; e += 64) part[e] = 0.0f;
    return;
  }
  f32x16 acc0[DAD_HT], acc1[DAD_HT];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    acc0[ht] = f32x16{};
    acc1[ht] = f32x16{};
  }
  // past the last frame: the utterance's last frame again, rows and noise (masked by vbits in the epilogue)
  const int tt = min(t, len - 1);
  const size_t row = (size_t)(a.rows[u] + (int64_t)tt);
  constexpr int CH = F16 ? 8 : 4;    // the lane's channels of one k-step
  NoiseSrc nz;
  nz.noise = a.noise;
  nz.nel = ((size_t)DAD_SLAB * (size_t)s0 + (size_t)tt) * DAD_D + CH * kh;
  nz.key = noise_key(a.skey, u, tt);
  nz.pair0 = noise_pair(tt, CH * kh);
  if constexpr (F16) {
    eval_slab_noise_f16<DT, EXPL>(a.store, row * DAD_D + 8 * kh, nz, a.w1h + (size_t)i * DAD_D + 8 * kh, acc0, acc1);
  } else {
    eval_slab_noise_f32<DT, EXPL>(a.store, row * DAD_D + 4 * kh, nz,
                                  a.params + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh, acc0, acc1);
  }
  // Both accumulators are read by every level's epilogue.  Left to itself the register allocator then keeps part
  // of them in VALU registers through the GEMM loop and spills the W1 fragments; pinning them to the accumulator
  // file here ends that (each epilogue copies the 32 values it reads).
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) asm volatile("" : "+a"(acc0[ht]), "+a"(acc1[ht]));
  eval_epilogue_noise<DAD_EN_MAX_LEVELS>(acc0, acc1, a.sigma, a.levels, a.params + DAD_OFF_B1, part, vbits);
}

// row-major fp16 copy of the network's W1
__global__ __launch_bounds__(256) void dad_noise_w1h(const float* params, uint16_t* w) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)DAD_H * DAD_D) return;
  w[i] = dad_half_bits(params[DAD_OFF_W1 + i], true);
}

__global__ __launch_bounds__(64 * kHeadWaves) void dad_noise_head(NoiseHeadArgs a) {
  DAD_GUARD_BLOCK(64 * kHeadWaves);
  const int lane = threadIdx.x & 63;
  const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kHeadWaves + (threadIdx.x >> 6)));
  if (u >= a.n) return;
  const int len = max(a.lens[u], 0);
  int s0 = a.slab_off[u], s1 = a.slab_off[u + 1];
  if (s0 < 0 || s1 > a.slabs || s1 - s0 != (len + DAD_SLAB - 1) / DAD_SLAB) s0 = s1 = 0;   // inconsistent table: a zero embedding
  f32x4 x0 = f32x4{0.f, 0.f, 0.f, 0.f};
  float lp0[DAD_C], p0[DAD_C];
  int pred0 = 0, brk = a.levels;
  bool any_bad = false;
  for (int k = 0; k < a.levels; ++k) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = s0; c < s1; ++c)
      s += *reinterpret_cast<const f32x4*>(a.part + ((size_t)c * a.levels + k) * DAD_H + 4 * lane);
    const size_t o = (size_t)k * a.n + u;
    bool bad = false;
    HeadVals hv;
    const int am = eval_head_pooled_v(s, (float)len, a.params, a.use_entropy, o, a.emb, a.logits, a.probs, a.score,
                                      a.ws_score, &bad, hv);
    any_bad = any_bad || bad;
    // log-softmax of this level's logits
    const float lse = logf(hv.se);
    float lp[DAD_C];
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) lp[c] = (hv.z[c] - hv.m) - lse;
    if (k == 0) {
      x0 = hv.x;
      pred0 = am;
#pragma unroll
      for (int c = 0; c < DAD_C; ++c) { lp0[c] = lp[c]; p0[c] = hv.p[c]; }
    }
    if (k > 0 && am != pred0 && brk == a.levels) brk = k;
    float q = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = hv.x[e] - x0[e];
      q += d * d;
    }
    const float drift = sqrtf(dad_wave_sum(q));
    float kl = 0.0f;
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) kl += p0[c] > 0.0f ? p0[c] * (lp0[c] - lp[c]) : 0.0f;
    if (lane == 0) {
      if (a.pred) a.pred[o] = am;
      if (a.drift) a.drift[o] = drift;
      if (a.kl) a.kl[o] = kl;
      a.ws_pred[o] = am;
      a.ws_drift[o] = drift;
      a.ws_kl[o] = kl;
    }
  }
  if (lane == 0) {
    if (a.break_level) a.break_level[u] = brk;
    a.ws_break[u] = brk;
    a.ws_bad[u] = any_bad ? 1 : 0;
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

__global__ __launch_bounds__(kResThreads) void dad_noise_result(NoiseResArgs a) {
  DAD_GUARD_BLOCK(kResThreads);
  __shared__ unsigned int cnt[DAD_EN_COUNTS];
  __shared__ double red[kResThreads];
  const int tid = threadIdx.x;
  if (tid < DAD_EN_COUNTS) cnt[tid] = 0u;
  __syncthreads();
  for (int u = tid; u < a.n; u += kResThreads) {
    const long y = a.labels ? (long)a.labels[u] : -1;
    const bool lab = y >= 0 && y < DAD_C;
    atomicAdd(&cnt[lab ? DAD_EN_N_LABELLED : DAD_EN_N_SKIPPED], 1u);
    if (a.ws_bad[u]) atomicAdd(&cnt[DAD_EN_N_NONFINITE], 1u);
    const int p0 = a.ws_pred[u], brk = a.ws_break[u];
    for (int k = 0; k < a.levels; ++k) {
      const int pk = a.ws_pred[(size_t)k * a.n + u];
      if (lab) atomicAdd(&cnt[DAD_EN_CONF + k * DAD_C * DAD_C + (int)y * DAD_C + pk], 1u);
      if (pk != p0) atomicAdd(&cnt[DAD_EN_FLIPS + k], 1u);
      if (brk > k) atomicAdd(&cnt[DAD_EN_SURVIVE + k], 1u);
    }
  }
  __syncthreads();
  if (tid < DAD_EN_COUNTS) {
    int64_t v = (int64_t)cnt[tid];
    if (tid == DAD_EN_N) v = a.n;
    if (tid == DAD_EN_LEVELS) v = a.levels;
    a.counts[tid] = v;
  }
  const float* src[3] = {a.ws_score, a.ws_drift, a.ws_kl};
  const int slot[3] = {DAD_EN_SUM_SCORE, DAD_EN_SUM_DRIFT, DAD_EN_SUM_KL};
  for (int q = 0; q < 3; ++q)
    for (int k = 0; k < DAD_EN_MAX_LEVELS; ++k) {
      double tot = 0.0;
      if (k < a.levels) {
        double s = 0.0;
        for (int u = tid; u < a.n; u += kResThreads) s += (double)src[q][(size_t)k * a.n + u];
        tot = block_sum_d(s, red);
      }
      if (tid == 0) a.sums[slot[q] + k] = tot;
    }
}

// the counter mode's normals in the explicit layout: one block per row of the [32 * slabs][768] array
__global__ __launch_bounds__(kDrawThreads) void dad_noise_draws(NoiseDrawArgs a) {
  DAD_GUARD_BLOCK(kDrawThreads);
  const int r = (int)blockIdx.x;     // < 32 * slabs < 2^31
  const int job = r / DAD_SLAB;
  if (job >= a.slabs) return;
  const int u = slab_owner(a.slab_off, a.n, job);
  const int c = job - a.slab_off[u];
  const int t = c * DAD_SLAB + (r % DAD_SLAB);
  const int d = 4 * (int)threadIdx.x;
  f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c >= 0 && t < a.lens[u]) z = noise_normal4(noise_key(a.skey, u, t), noise_pair(t, 0), d);
  *reinterpret_cast<f32x4*>(a.out + (size_t)r * DAD_D + d) = z;
}

struct NoiseWs {
  size_t part, pred, score, drift, kl, bad, brk, w1h, bytes;
};

NoiseWs noise_ws_layout(int64_t n, int64_t slabs, int levels, int precision) {
  NoiseWs w;
  size_t off = 0;
  const size_t sl = (size_t)(slabs > 0 ? slabs : 1), kn = (size_t)levels * (size_t)n;
  w.part = off;  off = dad_align(off + sizeof(float) * sl * (size_t)levels * DAD_H);
  w.pred = off;  off = dad_align(off + sizeof(int32_t) * kn);
  w.score = off; off = dad_align(off + sizeof(float) * kn);
  w.drift = off; off = dad_align(off + sizeof(float) * kn);
  w.kl = off;    off = dad_align(off + sizeof(float) * kn);
  w.bad = off;   off = dad_align(off + sizeof(int32_t) * (size_t)n);
  w.brk = off;   off = dad_align(off + sizeof(int32_t) * (size_t)n);
  w.w1h = off;   off = dad_align(off + (precision == DAD_PREC_FP16 ? sizeof(uint16_t) * DAD_H * DAD_D : 0));
  w.bytes = off;
  return w;
}

bool noise_shape_ok(int64_t n, int64_t slabs, int levels) {
  // the kernels index part[slab][level][256] and the [32 * slabs] noise rows with 32 bits
  return n >= 1 && n <= 0x7fffffffLL && slabs >= 0 && slabs <= n * (int64_t)(1 << 26) && slabs <= 0x7fffffffLL &&
         slabs * (int64_t)levels * DAD_H < (1LL << 31);
}

template <int DT>
void launch_encode(const NoiseEncArgs& ea, bool f16, bool expl, hipStream_t stream) {
  const dim3 grid((unsigned)((ea.slabs + kEncThreads / 64 - 1) / (kEncThreads / 64))), block(kEncThreads);
  if (f16) {
    if (expl) hipLaunchKernelGGL((dad_noise_encode<DT, true, true>), grid, block, 0, stream, ea);
    else hipLaunchKernelGGL((dad_noise_encode<DT, true, false>), grid, block, 0, stream, ea);
  } else {
    if (expl) hipLaunchKernelGGL((dad_noise_encode<DT, false, true>), grid, block, 0, stream, ea);
    else hipLaunchKernelGGL((dad_noise_encode<DT, false, false>), grid, block, 0, stream, ea);
  }
}

}  // namespace

extern "C" size_t dad_eval_noise_workspace_bytes(int64_t n, int64_t slabs, int levels, int precision) {
  if (levels < 1 || levels > DAD_EN_MAX_LEVELS || !noise_shape_ok(n, slabs, levels)) return 0;
  return noise_ws_layout(n, slabs, levels, precision).bytes;
}

extern "C" int dad_eval_noise(const dad_noise_args* args, void* workspace, void* stream_) {
  if (!args || !workspace) return DAD_E_ARG;
  if (!args->store || !args->rows || !args->lens || !args->slab_off || !args->params || !args->counts || !args->sums)
    return DAD_E_ARG;
  const int dt = args->store_dtype;
  if (dt != DAD_STORE_F32 && dt != DAD_STORE_F16 && dt != DAD_STORE_BF16) return DAD_E_ARG;
  if (args->levels < 1 || args->levels > DAD_EN_MAX_LEVELS) return DAD_E_ARG;
  for (int k = 0; k < args->levels; ++k)
    if (!std::isfinite(args->sigma[k]) || args->sigma[k] < 0.0f) return DAD_E_ARG;
  if (args->precision == DAD_PREC_BF16) return DAD_E_UNSUPPORTED;
  if (args->precision != DAD_PREC_FP32 && args->precision != DAD_PREC_FP16) return DAD_E_ARG;
  if (!noise_shape_ok(args->n, args->slabs, args->levels)) return DAD_E_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const bool f16 = args->precision == DAD_PREC_FP16;
  const int n = (int)args->n, K = args->levels;
  const NoiseWs L = noise_ws_layout(args->n, args->slabs, K, args->precision);
  char* ws = (char*)workspace;

  NoiseEncArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.store = args->store; ea.rows = args->rows; ea.lens = args->lens; ea.slab_off = args->slab_off;
  ea.n = n; ea.slabs = (int)args->slabs; ea.levels = K;
  ea.params = args->params;
  ea.w1h = (const uint16_t*)(ws + L.w1h);
  ea.noise = args->noise;
  ea.skey = dad_stream_key(args->seed, args->draw, DAD_RNG_EVAL_NOISE);
  for (int k = 0; k < K; ++k) ea.sigma[k] = args->sigma[k];
  ea.part = (float*)(ws + L.part);
  if (ea.slabs > 0) {
    if (f16) {
      hipLaunchKernelGGL(dad_noise_w1h, dim3((DAD_H * DAD_D + 255) / 256), dim3(256), 0, stream, args->params,
                         (uint16_t*)(ws + L.w1h));
      DAD_TRY(hipGetLastError());
    }
    const bool expl = args->noise != nullptr;
    switch (dt) {
      case DAD_STORE_F16: launch_encode<DAD_STORE_F16>(ea, f16, expl, stream); break;
      case DAD_STORE_BF16: launch_encode<DAD_STORE_BF16>(ea, f16, expl, stream); break;
      default: launch_encode<DAD_STORE_F32>(ea, f16, expl, stream); break;
    }
    DAD_TRY(hipGetLastError());
  }

  NoiseHeadArgs ha;
  memset(&ha, 0, sizeof(ha));
  ha.n = n; ha.slabs = ea.slabs; ha.levels = K; ha.use_entropy = args->use_entropy;
  ha.lens = args->lens; ha.slab_off = args->slab_off;
  ha.part = ea.part; ha.params = args->params;
  ha.emb = args->emb; ha.logits = args->logits; ha.probs = args->probs; ha.score = args->score; ha.pred = args->pred;
  ha.drift = args->drift; ha.kl = args->kl; ha.break_level = args->break_level;
  ha.ws_pred = (int32_t*)(ws + L.pred); ha.ws_score = (float*)(ws + L.score); ha.ws_drift = (float*)(ws + L.drift);
  ha.ws_kl = (float*)(ws + L.kl); ha.ws_bad = (int32_t*)(ws + L.bad); ha.ws_break = (int32_t*)(ws + L.brk);
  hipLaunchKernelGGL(dad_noise_head, dim3((unsigned)((n + kHeadWaves - 1) / kHeadWaves)), dim3(64 * kHeadWaves), 0,
                     stream, ha);
  DAD_TRY(hipGetLastError());

  NoiseResArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.n = n; ra.levels = K; ra.labels = args->labels;
  ra.ws_pred = ha.ws_pred; ra.ws_score = ha.ws_score; ra.ws_drift = ha.ws_drift; ra.ws_kl = ha.ws_kl;
  ra.ws_bad = ha.ws_bad; ra.ws_break = ha.ws_break;
  ra.counts = args->counts; ra.sums = args->sums;
  hipLaunchKernelGGL(dad_noise_result, dim3(1), dim3(kResThreads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_eval_noise_draws(const dad_noise_args* args, float* out, void* stream_) {
  if (!args || !out || !args->lens || !args->slab_off) return DAD_E_ARG;
  if (!noise_shape_ok(args->n, args->slabs, 1)) return DAD_E_SHAPE;
  if (args->slabs == 0) return DAD_OK;
  NoiseDrawArgs da;
  memset(&da, 0, sizeof(da));
  da.lens = args->lens; da.slab_off = args->slab_off;
  da.n = (int)args->n; da.slabs = (int)args->slabs;
  da.skey = dad_stream_key(args->seed, args->draw, DAD_RNG_EVAL_NOISE);
  da.out = out;
  hipLaunchKernelGGL(dad_noise_draws, dim3((unsigned)(da.slabs * DAD_SLAB)), dim3(kDrawThreads), 0, (hipStream_t)stream_,
                     da);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}
