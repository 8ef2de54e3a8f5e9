// Several networks on one split, store-fed: one call evaluates up to 8 checkpoints on every utterance of a
// FeatureStore split and leaves what a comparison of them reads in one result block (dad.h, "several networks on
// one split"): per-member confusion matrices, pairwise disagreement and McNemar cells, the correct-count histogram,
// and the float64 sums behind mean NLL, Brier score and entropy of every model and of their mean ensemble.
//
// dad_eval_split streams the whole of W1 per 32-frame slab, and that traffic, not the store or the matrix cores,
// sets its time.  The slab kernel here is built for W1 reuse: one wave runs ONE model on TWO consecutive slab jobs,
// so every W1 fragment it loads feeds two slabs' MFMAs (the two 128-register accumulator sets of dad_eval_encode's
// teacher instance, and half its W fragments).
//
// Launches, no host work in between:
//   dad_models_w1h      FP16 only: the K row-major fp16 copies of W1 (dad_eval_w1h's rounding).
//   dad_models_encode   wave j = p K + k runs model k on slab jobs 2p and 2p + 1 (consecutive waves share a slab
//                       pair's rows).  The two jobs may belong to different utterances: each has its own owner, row
//                       base and valid-row bits.  Within a slab the k order, the e order and the ht order are
//                       eval_slab_f32's / eval_slab_f16's and the epilogue is eval_epilogue, so part[k][slab][256]
//                       holds dad_eval_encode's bits for student = models[k].
//   dad_models_head     one wave per utterance walks the models in order: slab partials summed in slab order,
//                       eval_head_pooled_v, then the ensemble chain, the vote and the correct count.
//   dad_models_result   one workgroup: the DAD_EM_* block (integer LDS atomics fed by wave ballots; float64 sums by
//                       strided per-thread sums and a fixed LDS tree).
// No floating-point atomics anywhere.
#include <cmath>
#include <cstring>

#include "dad_common.h"
#include "dad_kernels.h"
#include "eval_rows.h"

namespace {

constexpr int kEncThreads = 256;     // 4 waves, one (model, slab pair) each
constexpr int kHeadWaves = 4;
constexpr int kResThreads = 256;
constexpr int kMaxK = DAD_EM_MAX_MODELS;
constexpr int kMembers = DAD_EM_MEMBERS;
static_assert(DAD_EM_HIST + kMaxK + 1 == DAD_EM_N && DAD_EM_NONFINITE + kMaxK == DAD_EM_K, "the DAD_EM_* layout");
static_assert(2 * kMembers <= 32, "dad_models_result packs a member's prediction into 2 bits of one word");

struct ModelsEncArgs {
  const void* store;
  const int64_t* rows; const int32_t* lens; const int32_t* slab_off;
  int n, slabs, K;
  const float* models[kMaxK];        // flat [W1|b1|W2|b2]
  const uint16_t* w1h;               // FP16: [K] row-major fp16 W1 copies
  float* part;                       // [K][slabs][256]
};

struct ModelsW1hArgs {
  const float* models[kMaxK];
  uint16_t* w1h;
};

struct ModelsHeadArgs {
  int n, slabs, K, use_entropy;
  const int32_t* lens; const int32_t* slab_off; const int64_t* labels;
  const float* part;
  const float* models[kMaxK];
  float wn[kMaxK];                   // normalised ensemble weights
  float* emb; float* logits; float* probs; float* score; int64_t* pred;
  float* ens_probs; float* ens_score; int64_t* ens_pred; int64_t* vote_pred; int32_t* votes; int32_t* n_correct;
  int32_t* ws_pred;                  // [K + 2][n]
  float* ws_probs;                   // [K + 1][n][4]
  float* ws_score;                   // [K + 1][n]
  int32_t* ws_bad;                   // [K][n]
  int32_t* ws_nc;                    // [n]
};

struct ModelsResArgs {
  int n, K;
  const int64_t* labels;
  const int32_t* ws_pred; const float* ws_probs; const float* ws_score; const int32_t* ws_bad; const int32_t* ws_nc;
  int64_t* counts; double* sums;
};

// eval_slab_f32 for two slabs on one W fragment: acc0 += x0 W1, acc1 += x1 W1.  Each accumulator sees the MFMAs of
// eval_slab_f32 in its order, so it holds the same bits.  The next step's two x chunks and the W1 fragments are
// fetched while this step's MFMAs run.
template <int DT>
__device__ __forceinline__ void models_pair_f32(const void* store, size_t xel0, size_t xel1, const float* W,
                                                f32x16 (&acc0)[DAD_HT], f32x16 (&acc1)[DAD_HT]) {
  Raw4<DT> xc0, xc1, xn0, xn1;
  f32x4 wc[DAD_HT], wn[DAD_HT];
  xc0.load(store, xel0);
  xc1.load(store, xel1);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 8) {
    const int dn = d0 + 8 < DAD_D ? d0 + 8 : d0;   // the last step reloads itself
    xn0.load(store, xel0 + dn);
    xn1.load(store, xel1 + dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D + dn);
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 x0 = xc0.get(), x1 = xc1.get();
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[e], wc[ht][e], acc0[ht], 0, 0, 0);
        acc1[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[e], wc[ht][e], acc1[ht], 0, 0, 0);
      }
    xc0 = xn0;
    xc1 = xn1;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// eval_slab_f16 for two slabs on one W fragment
template <int DT>
__device__ __forceinline__ void models_pair_f16(const void* store, size_t xel0, size_t xel1, const uint16_t* W,
                                                f32x16 (&acc0)[DAD_HT], f32x16 (&acc1)[DAD_HT]) {
  Raw8<DT> xc0, xc1, xn0, xn1;
  u32x4 wc[DAD_HT], wn[DAD_HT];
  xc0.load(store, xel0);
  xc1.load(store, xel1);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 16) {
    const int dn = d0 + 16 < DAD_D ? d0 + 16 : d0;
    xn0.load(store, xel0 + dn);
    xn1.load(store, xel1 + dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D + dn);
    __builtin_amdgcn_sched_barrier(0);
    const f16x8 x0 = __builtin_bit_cast(f16x8, xc0.frag());
    const f16x8 x1 = __builtin_bit_cast(f16x8, xc1.frag());
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) {
      const f16x8 w = __builtin_bit_cast(f16x8, wc[ht]);
      acc0[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0, w, acc0[ht], 0, 0, 0);
      acc1[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x1, w, acc1[ht], 0, 0, 0);
    }
    xc0 = xn0;
    xc1 = xn1;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// One slab job of a pair: its owner's length, the lane's frame and the valid-row bits (0 for a job that does not
// exist or whose table entry disagrees with the length: nothing of it is read)
struct SlabJob {
  int u, len, t;
  uint32_t vbits;
};
__device__ __forceinline__ SlabJob models_job(const ModelsEncArgs& a, int job, int i) {
  SlabJob s;
  s.u = 0; s.len = 0; s.t = 0; s.vbits = 0u;
  if (job < a.slabs) {
    s.u = slab_owner(a.slab_off, a.n, job);
    s.len = a.lens[s.u];
    const int c = job - a.slab_off[s.u];
    s.t = c * DAD_SLAB + i;
    s.vbits = (uint32_t)__ballot(s.t < s.len && c >= 0);
  }
  return s;
}

template <int DT, bool F16>
__global__ __launch_bounds__(kEncThreads) void dad_models_encode(ModelsEncArgs a) {
  DAD_GUARD_BLOCK(kEncThreads);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kEncThreads / 64) + (threadIdx.x >> 6)));
  const int p = w / a.K, k = w - p * a.K;
  const int j0 = 2 * p, j1 = 2 * p + 1;
  if (j0 >= a.slabs) return;
  const int i = lane & 31, kh = lane >> 5;
  const SlabJob s0 = models_job(a, j0, i), s1 = models_job(a, j1, i);
  const float* flat = a.models[k];
  f32x16 acc0[DAD_HT], acc1[DAD_HT];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    acc0[ht] = f32x16{};
    acc1[ht] = f32x16{};
  }
  if ((s0.vbits | s1.vbits) != 0u) {
    // past the last frame: the utterance's last row again (masked by vbits in the epilogue); a job without valid
    // rows reads its partner's row, which is in range, and its accumulator is never used
    size_t r0 = 0, r1 = 0;
    if (s0.vbits != 0u) r0 = (size_t)(a.rows[s0.u] + (int64_t)min(s0.t, s0.len - 1));
    if (s1.vbits != 0u) r1 = (size_t)(a.rows[s1.u] + (int64_t)min(s1.t, s1.len - 1));
    if (s0.vbits == 0u) r0 = r1;
    if (s1.vbits == 0u) r1 = r0;
    if constexpr (F16) {
      const uint16_t* W = a.w1h + (size_t)k * DAD_H * DAD_D + (size_t)i * DAD_D + 8 * kh;
      models_pair_f16<DT>(a.store, r0 * DAD_D + 8 * kh, r1 * DAD_D + 8 * kh, W, acc0, acc1);
    } else {
      const float* W = flat + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh;
      models_pair_f32<DT>(a.store, r0 * DAD_D + 4 * kh, r1 * DAD_D + 4 * kh, W, acc0, acc1);
    }
  }
  float* part = a.part + ((size_t)k * a.slabs + j0) * DAD_H;
  eval_epilogue(acc0, flat + DAD_OFF_B1, part, s0.vbits);
  if (j1 < a.slabs) eval_epilogue(acc1, flat + DAD_OFF_B1, part + DAD_H, s1.vbits);
}

// row-major fp16 copies of the K networks' W1 (blockIdx.y: the model)
__global__ __launch_bounds__(256) void dad_models_w1h(ModelsW1hArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)DAD_H * DAD_D) return;
  const int k = blockIdx.y;
  a.w1h[(size_t)k * DAD_H * DAD_D + i] = dad_half_bits(a.models[k][DAD_OFF_W1 + i], true);
}

__global__ __launch_bounds__(64 * kHeadWaves) void dad_models_head(ModelsHeadArgs a) {
  DAD_GUARD_BLOCK(64 * kHeadWaves);
  const int lane = threadIdx.x & 63;
  const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kHeadWaves + (threadIdx.x >> 6)));
  if (u >= a.n) return;
  const int len = max(a.lens[u], 0);
  int s0 = a.slab_off[u], s1 = a.slab_off[u + 1];
  if (s0 < 0 || s1 > a.slabs || s1 - s0 != (len + DAD_SLAB - 1) / DAD_SLAB) s0 = s1 = 0;   // inconsistent table: a zero embedding
  const long y = a.labels ? (long)a.labels[u] : -1;
  const bool lab = y >= 0 && y < DAD_C;
  float e[DAD_C];
  int vt[DAD_C];
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) { e[c] = 0.0f; vt[c] = 0; }
  int nc = 0;
  for (int k = 0; k < a.K; ++k) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = s0; c < s1; ++c)
      s += *reinterpret_cast<const f32x4*>(a.part + ((size_t)k * a.slabs + c) * DAD_H + 4 * lane);
    const size_t o = (size_t)k * a.n + u;
    bool bad = false;
    HeadVals hv;
    const int am = eval_head_pooled_v(s, (float)len, a.models[k], a.use_entropy, o, a.emb, a.logits, a.probs, a.score,
                                      a.ws_score, &bad, hv);
    const float wk = a.wn[k];
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) {
      e[c] = fmaf(wk, hv.p[c], e[c]);
      vt[c] += am == c ? 1 : 0;
    }
    nc += (lab && am == (int)y) ? 1 : 0;
    if (lane == 0) {
      if (a.pred) a.pred[o] = am;
      a.ws_pred[o] = am;
      a.ws_bad[o] = bad ? 1 : 0;
#pragma unroll
      for (int c = 0; c < DAD_C; ++c) a.ws_probs[o * DAD_C + c] = hv.p[c];
    }
  }
  // the mean ensemble: first-maximum argmax and the head's certainty formula on its probabilities
  float m = e[0], ent = 0.0f;
  int am = 0, vm = 0, vbest = vt[0];
#pragma unroll
  for (int c = 1; c < DAD_C; ++c) {
    if (e[c] > m) { m = e[c]; am = c; }
    if (vt[c] > vbest) { vbest = vt[c]; vm = c; }      // ties to the lowest class
  }
  float pmax = 0.0f;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    pmax = fmaxf(pmax, e[c]);
    ent -= e[c] * log2f(e[c] + 1e-8f);
  }
  const float sc = a.use_entropy ? pmax * (1.0f - ent / 2.0f) : pmax;
  if (lane == 0) {
    const size_t oe = (size_t)a.K * a.n + u, ov = (size_t)(a.K + 1) * a.n + u;
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) {
      if (a.ens_probs) a.ens_probs[(size_t)u * DAD_C + c] = e[c];
      if (a.votes) a.votes[(size_t)u * DAD_C + c] = vt[c];
      a.ws_probs[oe * DAD_C + c] = e[c];
    }
    if (a.ens_score) a.ens_score[u] = sc;
    if (a.ens_pred) a.ens_pred[u] = am;
    if (a.vote_pred) a.vote_pred[u] = vm;
    if (a.n_correct) a.n_correct[u] = lab ? nc : -1;
    a.ws_score[oe] = sc;
    a.ws_pred[oe] = am;
    a.ws_pred[ov] = vm;
    a.ws_nc[u] = lab ? nc : -1;
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

__global__ __launch_bounds__(kResThreads) void dad_models_result(ModelsResArgs a) {
  DAD_GUARD_BLOCK(kResThreads);
  __shared__ unsigned int cnt[DAD_EM_COUNTS];
  __shared__ double red[kResThreads];
  const int tid = threadIdx.x, lane = tid & 63;
  const int M = a.K + 2;
  for (int q = tid; q < DAD_EM_COUNTS; q += kResThreads) cnt[q] = 0u;
  __syncthreads();
  // 64 utterances per wave and pass: a member's prediction is 2 bits of pk; a pair's counts are wave ballots, so
  // one lane adds them to LDS
  for (int base = tid - lane; base < a.n; base += kResThreads) {
    const int u = base + lane;
    const bool in = u < a.n;
    const long y = (in && a.labels) ? (long)a.labels[u] : -1;
    const bool lab = in && y >= 0 && y < DAD_C;
    uint32_t pk = 0u;
    for (int m = 0; m < M; ++m) {
      const int pm = in ? a.ws_pred[(size_t)m * a.n + u] : 0;
      pk |= (uint32_t)pm << (2 * m);
      if (lab) atomicAdd(&cnt[DAD_EM_CONF + m * DAD_C * DAD_C + (int)y * DAD_C + pm], 1u);
    }
    if (in) atomicAdd(&cnt[lab ? DAD_EM_N_LABELLED : DAD_EM_N_SKIPPED], 1u);
    if (lab) atomicAdd(&cnt[DAD_EM_HIST + a.ws_nc[u]], 1u);
    for (int k = 0; k < a.K; ++k) {
      const unsigned int nb = (unsigned int)__popcll(__ballot(in && a.ws_bad[(size_t)k * a.n + u] != 0));
      if (lane == 0 && nb) atomicAdd(&cnt[DAD_EM_NONFINITE + k], nb);
    }
    for (int ma = 0; ma < M; ++ma) {
      const int pa = (int)((pk >> (2 * ma)) & 3u);
      const bool ra = lab && pa == (int)y;
      for (int mb = 0; mb < M; ++mb) {
        const int pb = (int)((pk >> (2 * mb)) & 3u);
        const unsigned int dis = (unsigned int)__popcll(__ballot(in && pa != pb));
        const unsigned int only = (unsigned int)__popcll(__ballot(ra && (ma == mb || pb != (int)y)));
        if (lane == 0) {
          if (dis) atomicAdd(&cnt[DAD_EM_DISAGREE + ma * kMembers + mb], dis);
          if (only) atomicAdd(&cnt[DAD_EM_ONLY + ma * kMembers + mb], only);
        }
      }
    }
  }
  __syncthreads();
  for (int q = tid; q < DAD_EM_COUNTS; q += kResThreads) {
    int64_t v = (int64_t)cnt[q];
    if (q == DAD_EM_N) v = a.n;
    if (q == DAD_EM_K) v = a.K;
    a.counts[q] = v;
  }
  // per member with probabilities: float64 terms from the float32 values, strided per-thread sums and a fixed tree
  for (int m = 0; m < kMembers; ++m) {
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    if (m <= a.K) {
      double sc = 0.0, en = 0.0, nl = 0.0, br = 0.0;
      for (int u = tid; u < a.n; u += kResThreads) {
        const size_t o = (size_t)m * a.n + u;
        const f32x4 pf = *reinterpret_cast<const f32x4*>(a.ws_probs + o * DAD_C);
        const long y = a.labels ? (long)a.labels[u] : -1;
        const bool lab = y >= 0 && y < DAD_C;
        sc += (double)a.ws_score[o];
        double h = 0.0, b = 0.0, py = 1.0;
#pragma unroll
        for (int c = 0; c < DAD_C; ++c) {
          const double pc = (double)pf[c];
          h -= pc > 0.0 ? pc * log(pc) : 0.0;
          const double d = pc - ((long)c == y ? 1.0 : 0.0);
          b += d * d;
          if ((long)c == y) py = pc;
        }
        en += h;
        if (lab) {
          nl += -log(py);
          br += b;
        }
      }
      tot[0] = block_sum_d(sc, red);
      tot[1] = block_sum_d(en, red);
      tot[2] = block_sum_d(nl, red);
      tot[3] = block_sum_d(br, red);
    }
    if (tid == 0) {
      a.sums[DAD_EM_SUM_SCORE + m] = tot[0];
      a.sums[DAD_EM_SUM_ENTROPY + m] = tot[1];
      a.sums[DAD_EM_SUM_NLL + m] = tot[2];
      a.sums[DAD_EM_SUM_BRIER + m] = tot[3];
    }
  }
}

struct ModelsWs {
  size_t part, pred, probs, score, bad, nc, w1h, bytes;
};

ModelsWs models_ws_layout(int64_t n, int64_t slabs, int K, int precision) {
  ModelsWs w;
  size_t off = 0;
  const size_t sl = (size_t)(slabs > 0 ? slabs : 1), nn = (size_t)n, k = (size_t)K;
  w.part = off;  off = dad_align(off + sizeof(float) * k * sl * DAD_H);
  w.pred = off;  off = dad_align(off + sizeof(int32_t) * (k + 2) * nn);
  w.probs = off; off = dad_align(off + sizeof(float) * (k + 1) * nn * DAD_C);
  w.score = off; off = dad_align(off + sizeof(float) * (k + 1) * nn);
  w.bad = off;   off = dad_align(off + sizeof(int32_t) * k * nn);
  w.nc = off;    off = dad_align(off + sizeof(int32_t) * nn);
  w.w1h = off;   off = dad_align(off + (precision == DAD_PREC_FP16 ? sizeof(uint16_t) * k * DAD_H * DAD_D : 0));
  w.bytes = off;
  return w;
}

bool models_shape_ok(int64_t n, int64_t slabs, int K) {
  // the kernels index part[k][slab][256] and the K * ceil(slabs / 2) wave jobs with 32 bits
  return n >= 1 && n <= 0x7fffffffLL && slabs >= 0 && slabs <= n * (int64_t)(1 << 26) && slabs <= 0x7fffffffLL &&
         slabs * (int64_t)K * DAD_H < (1LL << 31);
}

template <int DT>
void launch_encode(const ModelsEncArgs& ea, bool f16, hipStream_t stream) {
  const int64_t waves = (int64_t)((ea.slabs + 1) / 2) * ea.K;
  const dim3 grid((unsigned)((waves + kEncThreads / 64 - 1) / (kEncThreads / 64))), block(kEncThreads);
  if (f16) hipLaunchKernelGGL((dad_models_encode<DT, true>), grid, block, 0, stream, ea);
  else hipLaunchKernelGGL((dad_models_encode<DT, false>), grid, block, 0, stream, ea);
}

}  // namespace

extern "C" size_t dad_eval_models_workspace_bytes(int64_t n, int64_t slabs, int K, int precision) {
  if (K < 1 || K > kMaxK || !models_shape_ok(n, slabs, K)) return 0;
  return models_ws_layout(n, slabs, K, precision).bytes;
}

extern "C" int dad_eval_models(const dad_models_args* args, void* workspace, void* stream_) {
  if (!args || !workspace) return DAD_E_ARG;
  if (!args->store || !args->rows || !args->lens || !args->slab_off || !args->counts || !args->sums) return DAD_E_ARG;
  const int dt = args->store_dtype;
  if (dt != DAD_STORE_F32 && dt != DAD_STORE_F16 && dt != DAD_STORE_BF16) return DAD_E_ARG;
  const int K = args->K;
  if (K < 1 || K > kMaxK) return DAD_E_ARG;
  double wsum = 0.0;
  for (int k = 0; k < K; ++k) {
    if (!args->models[k]) return DAD_E_ARG;
    if (!std::isfinite(args->weight[k]) || args->weight[k] < 0.0f) return DAD_E_ARG;
    wsum += (double)args->weight[k];
  }
  if (!(wsum > 0.0)) return DAD_E_ARG;
  if (args->precision == DAD_PREC_BF16) return DAD_E_UNSUPPORTED;
  if (args->precision != DAD_PREC_FP32 && args->precision != DAD_PREC_FP16) return DAD_E_ARG;
  if (!models_shape_ok(args->n, args->slabs, K)) return DAD_E_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const bool f16 = args->precision == DAD_PREC_FP16;
  const int n = (int)args->n;
  const ModelsWs L = models_ws_layout(args->n, args->slabs, K, args->precision);
  char* ws = (char*)workspace;

  ModelsEncArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.store = args->store; ea.rows = args->rows; ea.lens = args->lens; ea.slab_off = args->slab_off;
  ea.n = n; ea.slabs = (int)args->slabs; ea.K = K;
  for (int k = 0; k < K; ++k) ea.models[k] = args->models[k];
  ea.w1h = (const uint16_t*)(ws + L.w1h);
  ea.part = (float*)(ws + L.part);
  if (ea.slabs > 0) {
    if (f16) {
      ModelsW1hArgs wa;
      memset(&wa, 0, sizeof(wa));
      for (int k = 0; k < K; ++k) wa.models[k] = args->models[k];
      wa.w1h = (uint16_t*)(ws + L.w1h);
      hipLaunchKernelGGL(dad_models_w1h, dim3((DAD_H * DAD_D + 255) / 256, K), dim3(256), 0, stream, wa);
      DAD_TRY(hipGetLastError());
    }
    switch (dt) {
      case DAD_STORE_F16: launch_encode<DAD_STORE_F16>(ea, f16, stream); break;
      case DAD_STORE_BF16: launch_encode<DAD_STORE_BF16>(ea, f16, stream); break;
      default: launch_encode<DAD_STORE_F32>(ea, f16, stream); break;
    }
    DAD_TRY(hipGetLastError());
  }

  ModelsHeadArgs ha;
  memset(&ha, 0, sizeof(ha));
  ha.n = n; ha.slabs = ea.slabs; ha.K = K; ha.use_entropy = args->use_entropy;
  ha.lens = args->lens; ha.slab_off = args->slab_off; ha.labels = args->labels;
  ha.part = ea.part;
  for (int k = 0; k < K; ++k) {
    ha.models[k] = args->models[k];
    ha.wn[k] = (float)((double)args->weight[k] / wsum);
  }
  ha.emb = args->emb; ha.logits = args->logits; ha.probs = args->probs; ha.score = args->score; ha.pred = args->pred;
  ha.ens_probs = args->ens_probs; ha.ens_score = args->ens_score; ha.ens_pred = args->ens_pred;
  ha.vote_pred = args->vote_pred; ha.votes = args->votes; ha.n_correct = args->n_correct;
  ha.ws_pred = (int32_t*)(ws + L.pred); ha.ws_probs = (float*)(ws + L.probs); ha.ws_score = (float*)(ws + L.score);
  ha.ws_bad = (int32_t*)(ws + L.bad); ha.ws_nc = (int32_t*)(ws + L.nc);
  hipLaunchKernelGGL(dad_models_head, dim3((unsigned)((n + kHeadWaves - 1) / kHeadWaves)), dim3(64 * kHeadWaves), 0,
                     stream, ha);
  DAD_TRY(hipGetLastError());

  ModelsResArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.n = n; ra.K = K; ra.labels = args->labels;
  ra.ws_pred = ha.ws_pred; ra.ws_probs = ha.ws_probs; ra.ws_score = ha.ws_score; ra.ws_bad = ha.ws_bad;
  ra.ws_nc = ha.ws_nc;
  ra.counts = args->counts; ra.sums = args->sums;
  hipLaunchKernelGGL(dad_models_result, dim3(1), dim3(kResThreads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}
