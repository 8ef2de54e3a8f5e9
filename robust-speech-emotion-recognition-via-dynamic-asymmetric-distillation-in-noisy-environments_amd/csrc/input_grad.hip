// Gradient of the eval-mode forward with respect to the stored rows, store-fed: for every utterance of a
// FeatureStore split and a caller's logit cotangent dz_u[4], G = (ReLU' (.) g_u) W1 with g_u = W2^T dz_u / len, and
// from it the signed step clamp(delta + alpha sgn(G), +-radius) of FGSM / PGD (dad.h, "input gradients of a split").
// The caller supplies dz: softmax(z) - onehot(target) makes G the gradient of PLAIN cross-entropy; the trainer's
// loss is label-smoothed and is not what the attacks here ascend.
//
// One launch (plus the two fp16 copies of W1 in FP16).  dad_noise_encode's work unit: one wave = one 32-frame slab
// against all 256 hidden units, four waves per workgroup, rows read in place.  Per slab:
//   forward    pre = (x + delta) W1^T by eval_rows.h's loops (delta == NULL: eval_slab_f32 / eval_slab_f16 themselves,
//              so the accumulators hold dad_eval_split's bits).
//   ReLU'      lane (j, kh) of accumulator register r holds hidden unit j of two rows, so one __ballot of
//              pre + b1 > 0 is the 32 hidden-unit bits of those two rows: 128 ballots are the bit matrix
//              [32 rows][8 words], already transposed.  Each word is kept by the lane whose row it is and parked in
//              LDS (1 KB per wave); rows past the utterance's length park zeros (selection, no product with 0).
//   g_u        256 floats per wave in LDS, fp32 in a fixed order: s = W2^T dz (one product and three fmas), / len.
//   backward   G = (m (.) g_u) W1: the A fragment is selected in registers from the lane's mask word and g_u, the B
//              fragment is W1[j][d0 + i].  The 24 column tiles of 32 channels need 384 accumulator registers, more
//              than the 256 of the accumulator file, so they are walked in 3 groups of 8 (the 128 registers the
//              forward just released); W1 is read again from L2 for every group.
//   epilogue   per element in the explicit layout [32 * slabs][768]: grad, the step, |G| into the frame's L1 sum
//              (per-lane sums in tile order, then a fixed xor tree over the 32 lanes of a row half).
// Counts by one integer atomic per wave and slot.  No floating-point atomics anywhere.
#include <cmath>
#include <cstring>

#include "dad_common.h"
#include "dad_kernels.h"
#include "eval_rows.h"

namespace {

constexpr int kIgThreads = 256;      // 4 waves, one slab each
constexpr int kIgWaves = kIgThreads / 64;
constexpr int kColTiles = DAD_D / 32;             // 24
constexpr int kGroupTiles = 8;                    // column tiles whose accumulators are live together
constexpr int kGroups = kColTiles / kGroupTiles;  // 3
static_assert(kColTiles % kGroupTiles == 0, "column groups");
constexpr int kScaleExp = 14;        // FP16: max |c s| lies in [2^14, 2^15)
constexpr int kScaleExpMax = 100;

struct IgArgs {
  const void* store;
  const int64_t* rows; const int32_t* lens; const int32_t* slab_off;
  int n, slabs;
  const float* params;               // flat [W1|b1|W2|b2]
  const uint16_t* w1h;               // FP16: row-major fp16 W1 copy [256][768]
  const uint16_t* w1t;               // FP16: transposed fp16 W1 copy [768][256]
  const float* dz;                   // [n][4]
  const float* delta_in;             // [32 * slabs][768] or NULL
  float* grad; float* delta_out; float* frame_l1;
  unsigned long long* counts;
  float alpha, radius;
};

// fp16 copies of W1: row-major for the forward, transposed for the data-gradient GEMM
__global__ __launch_bounds__(256) void dad_ig_w1h(const float* params, uint16_t* w, uint16_t* wt) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)DAD_H * DAD_D) return;
  const uint16_t h = dad_half_bits(params[DAD_OFF_W1 + e], true);
  const size_t j = e / DAD_D, d = e % DAD_D;
  w[e] = h;
  wt[d * DAD_H + j] = h;
}

__device__ __forceinline__ uint32_t pair_mask(uint32_t bits) {   // bits 0, 1 -> the two halves of a word
  return ((bits & 1u) ? 0x0000ffffu : 0u) | ((bits & 2u) ? 0xffff0000u : 0u);
}

template <int DT, bool F16, bool HASD>
__global__ __launch_bounds__(kIgThreads) void dad_input_grad_slab(IgArgs a) {
  DAD_GUARD_BLOCK(kIgThreads);
  __shared__ __attribute__((aligned(16))) uint32_t s_mask[kIgWaves][DAD_SLAB * DAD_HT];
  __shared__ __attribute__((aligned(16))) uint32_t s_g[kIgWaves][DAD_H];        // FP32: g_u as floats; FP16: c_u s_u as 256 halves
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kIgWaves + wv));
  if (job >= a.slabs) return;
  const int u = slab_owner(a.slab_off, a.n, job);
  const int len = a.lens[u];
  const int s0 = a.slab_off[u];
  const int c = job - s0;
  const int i = lane & 31, kh = lane >> 5;
  const int t = c * DAD_SLAB + i;
  const uint32_t vbits = (uint32_t)__ballot(t < len && c >= 0);
  const size_t out0 = (size_t)job * DAD_SLAB;      // the slab's first row in the explicit layout
  if (vbits == 0u) {                 // a table that disagrees with lens reads nothing and writes zeros
    for (int r = 0; r < DAD_SLAB; ++r)
      for (int d = lane; d < DAD_D; d += 64) {
        const size_t el = (out0 + r) * DAD_D + d;
        if (a.grad) a.grad[el] = 0.0f;
        if (a.delta_out) a.delta_out[el] = 0.0f;
      }
    if (a.frame_l1 && lane < DAD_SLAB) a.frame_l1[out0 + lane] = 0.0f;
    return;
  }
  uint32_t* mask = s_mask[wv];
  uint32_t* gl = s_g[wv];
  const float lenf = fmaxf((float)len, 1.0f);

  // ---- g_u (fixed order) ---------------------------------------------------------------------------------
  float invc = 1.0f;
  {
    const float* w2 = a.params + DAD_OFF_W2;
    const float* dz = a.dz + (size_t)u * DAD_C;
    const float z0 = dz[0], z1 = dz[1], z2 = dz[2], z3 = dz[3];
    f32x4 s;
    const f32x4 wa = *reinterpret_cast<const f32x4*>(w2 + 4 * lane);
    const f32x4 wb = *reinterpret_cast<const f32x4*>(w2 + DAD_H + 4 * lane);
    const f32x4 wc = *reinterpret_cast<const f32x4*>(w2 + 2 * DAD_H + 4 * lane);
    const f32x4 wd = *reinterpret_cast<const f32x4*>(w2 + 3 * DAD_H + 4 * lane);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float p = wa[e] * z0;
      p = fmaf(wb[e], z1, p);
      p = fmaf(wc[e], z2, p);
      p = fmaf(wd[e], z3, p);
      s[e] = p;
    }
    if constexpr (F16) {
      // c_u: the power of two that puts max |s| into [2^14, 2^15), so no g of a long utterance is an fp16 subnormal
      float m = fmaxf(fmaxf(fabsf(s[0]), fabsf(s[1])), fmaxf(fabsf(s[2]), fabsf(s[3])));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      int ex = 0;
      if (m > 0.0f && m <= 3.402823466e38f) ex = min(kScaleExp - ilogbf(m), kScaleExpMax);
      const float cu = ldexpf(1.0f, ex);
      invc = ldexpf(1.0f, -ex);
      gl[2 * lane] = dad_pack2<true>(s[0] * cu, s[1] * cu);
      gl[2 * lane + 1] = dad_pack2<true>(s[2] * cu, s[3] * cu);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) gl[4 * lane + e] = __float_as_uint(s[e] / lenf);
    }
  }

  // ---- forward GEMM and the ReLU' bit matrix ------------------------------------------------------------------
  {
    f32x16 acc[DAD_HT];
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) acc[ht] = f32x16{};
    // past the last frame: the utterance's last frame again, rows and delta (masked below)
    const int tt = min(t, len - 1);
    const size_t row = (size_t)(a.rows[u] + (int64_t)tt);
    constexpr int CH = F16 ? 8 : 4;  // the lane's channels of one k-step
    const size_t del = ((size_t)DAD_SLAB * (size_t)s0 + (size_t)tt) * DAD_D + CH * kh;
    if constexpr (F16) {
      const uint16_t* W = a.w1h + (size_t)i * DAD_D + 8 * kh;
      if constexpr (HASD) eval_slab_delta_f16<DT>(a.store, row * DAD_D + 8 * kh, a.delta_in, del, W, acc);
      else eval_slab_f16<DT, false>(a.store, row * DAD_D + 8 * kh, W, nullptr, acc, acc);
    } else {
      const float* W = a.params + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh;
      if constexpr (HASD) eval_slab_delta_f32<DT>(a.store, row * DAD_D + 4 * kh, a.delta_in, del, W, acc);
      else eval_slab_f32<DT, false>(a.store, row * DAD_D + 4 * kh, W, nullptr, acc, acc);
    }
    const float* b1 = a.params + DAD_OFF_B1;
    const bool rowv = (vbits >> i) & 1u;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) {
      const float bh = b1[ht * 32 + i];
      uint32_t w = 0u;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned long long b = __ballot(acc[ht][r] + bh > 0.0f);   // torch's ReLU': 0 at 0 (and at a NaN)
        const uint32_t half = kh ? (uint32_t)(b >> 32) : (uint32_t)b;
        w = (i == dad_acc_row(r, kh)) ? half : w;
      }
      // the lanes whose row lies in their own half of the accumulator rows hold that row's word of tile ht
      if (((i >> 2) & 1) == kh) mask[i * DAD_HT + ht] = rowv ? w : 0u;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- data-gradient GEMM in column groups, and the epilogue ----------------------------------------------
  float l1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) l1[r] = 0.0f;
  unsigned int n_bad = 0u, n_zero = 0u;
  const float alpha = a.alpha, radius = a.radius;
  for (int g = 0; g < kGroups; ++g) {
    const int d0 = g * kGroupTiles * 32;
    f32x16 acc[kGroupTiles];
#pragma unroll
    for (int ct = 0; ct < kGroupTiles; ++ct) acc[ct] = f32x16{};
    if constexpr (F16) {
      // k-step s: hidden units 16 s + 8 kh + jj; B = W1T[d0 + 32 ct + i][those 8]
      const uint16_t* B = a.w1t + (size_t)(d0 + i) * DAD_H + 8 * kh;
      u32x4 bc[kGroupTiles], bn[kGroupTiles];
#pragma unroll
      for (int ct = 0; ct < kGroupTiles; ++ct) bc[ct] = *reinterpret_cast<const u32x4*>(B + (size_t)ct * 32 * DAD_H);
      for (int s = 0; s < DAD_H / 16; ++s) {
        const int sn = s + 1 < DAD_H / 16 ? s + 1 : s;   // the last step reloads itself
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct)
          bn[ct] = *reinterpret_cast<const u32x4*>(B + (size_t)ct * 32 * DAD_H + 16 * sn);
        const uint32_t word = mask[i * DAD_HT + (s >> 1)];
        const uint32_t bits = (word >> ((s & 1) * 16 + 8 * kh)) & 0xffu;
        u32x4 hv = *reinterpret_cast<const u32x4*>(gl + 8 * s + 4 * kh);
#pragma unroll
        for (int p = 0; p < 4; ++p) hv[p] &= pair_mask(bits >> (2 * p));
        __builtin_amdgcn_sched_barrier(0);
        const f16x8 av = __builtin_bit_cast(f16x8, hv);
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, __builtin_bit_cast(f16x8, bc[ct]), acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct) bc[ct] = bn[ct];
      }
    } else {
      // k-step (j0, e, kh): hidden unit j0 + 4 kh + e; B = W1[that unit][d0 + 32 ct + i]
      const float* B = a.params + DAD_OFF_W1 + (size_t)(4 * kh) * DAD_D + d0 + i;
      float bc[kGroupTiles][4], bn[kGroupTiles][4];
#pragma unroll
      for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) bc[ct][e] = B[(size_t)e * DAD_D + ct * 32];
      for (int j0 = 0; j0 < DAD_H; j0 += 8) {
        const int jn = j0 + 8 < DAD_H ? j0 + 8 : j0;     // the last step reloads itself
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) bn[ct][e] = B[(size_t)(jn + e) * DAD_D + ct * 32];
        const uint32_t word = mask[i * DAD_HT + (j0 >> 5)];
        const uint32_t bits = (word >> ((j0 & 31) + 4 * kh)) & 0xfu;
        const u32x4 gv = *reinterpret_cast<const u32x4*>(gl + j0 + 4 * kh);
        float av[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = ((bits >> e) & 1u) ? __uint_as_float(gv[e]) : 0.0f;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bc[ct][e], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) bc[ct][e] = bn[ct][e];
      }
    }
    // lane (i, kh) of register r holds G[row dad_acc_row(r, kh)][d0 + 32 ct + i]; delta_in's element is read and
    // delta_out's written by this lane alone, so the two may be the same array
#pragma unroll
    for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rw = dad_acc_row(r, kh);
        const bool v = (vbits >> rw) & 1u;
        const size_t el = (out0 + rw) * DAD_D + d0 + ct * 32 + i;
        float G = acc[ct][r];
        if constexpr (F16) G = (G * invc) / lenf;
        const bool fin = fabsf(G) <= 3.402823466e38f;
        n_bad += (v && !fin) ? 1u : 0u;
        n_zero += (v && G == 0.0f) ? 1u : 0u;
        l1[r] += v ? fabsf(G) : 0.0f;
        if (a.grad) a.grad[el] = v ? G : 0.0f;
        if (a.delta_out) {
          float dl = 0.0f;
          if constexpr (HASD) dl = v ? a.delta_in[el] : 0.0f;
          float st = dl;
          if (fin && G > 0.0f) st = dl + alpha;
          if (fin && G < 0.0f) st = dl - alpha;
          st = fminf(fmaxf(st, -radius), radius);
          a.delta_out[el] = v ? st : 0.0f;
        }
      }
  }
  if (a.frame_l1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = l1[r];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (i == 0) a.frame_l1[out0 + dad_acc_row(r, kh)] = s;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_bad += __shfl_xor(n_bad, o, 64);
    n_zero += __shfl_xor(n_zero, o, 64);
  }
  if (lane == 0) {
    atomicAdd(a.counts + DAD_IG_FRAMES, (unsigned long long)__popc(vbits));
    if (n_bad) atomicAdd(a.counts + DAD_IG_NONFINITE, (unsigned long long)n_bad);
    if (n_zero) atomicAdd(a.counts + DAD_IG_ZERO, (unsigned long long)n_zero);
  }
}

struct IgWs {
  size_t w1h, w1t, bytes;
};

IgWs ig_ws_layout(int precision) {
  IgWs w;
  size_t off = 0;
  const size_t wb = precision == DAD_PREC_FP16 ? sizeof(uint16_t) * DAD_H * DAD_D : 0;
  w.w1h = off; off = dad_align(off + wb);
  w.w1t = off; off = dad_align(off + wb);
  w.bytes = off > 0 ? off : 256;
  return w;
}

bool ig_shape_ok(int64_t n, int64_t slabs) {
  return n >= 1 && n <= 0x7fffffffLL && slabs >= 0 && slabs <= n * (int64_t)(1 << 26) && slabs <= 0x7fffffffLL;
}

template <int DT>
void launch_slab(const IgArgs& ia, bool f16, hipStream_t stream) {
  const dim3 grid((unsigned)((ia.slabs + kIgWaves - 1) / kIgWaves)), block(kIgThreads);
  const bool hasd = ia.delta_in != nullptr;
  if (f16) {
    if (hasd) hipLaunchKernelGGL((dad_input_grad_slab<DT, true, true>), grid, block, 0, stream, ia);
    else hipLaunchKernelGGL((dad_input_grad_slab<DT, true, false>), grid, block, 0, stream, ia);
  } else {
    if (hasd) hipLaunchKernelGGL((dad_input_grad_slab<DT, false, true>), grid, block, 0, stream, ia);
    else hipLaunchKernelGGL((dad_input_grad_slab<DT, false, false>), grid, block, 0, stream, ia);
  }
}

}  // namespace

extern "C" size_t dad_input_grad_workspace_bytes(int64_t n, int64_t slabs, int precision) {
  if (!ig_shape_ok(n, slabs)) return 0;
  return ig_ws_layout(precision).bytes;
}

extern "C" int dad_input_grad(const dad_input_grad_args* args, void* workspace, void* stream_) {
  if (!args || !workspace) return DAD_E_ARG;
  if (!args->store || !args->rows || !args->lens || !args->slab_off || !args->params || !args->dz || !args->counts)
    return DAD_E_ARG;
  const int dt = args->store_dtype;
  if (dt != DAD_STORE_F32 && dt != DAD_STORE_F16 && dt != DAD_STORE_BF16) return DAD_E_ARG;
  if (!std::isfinite(args->alpha) || !(args->radius >= 0.0f)) return DAD_E_ARG;
  if (args->precision == DAD_PREC_BF16) return DAD_E_UNSUPPORTED;
  if (args->precision != DAD_PREC_FP32 && args->precision != DAD_PREC_FP16) return DAD_E_ARG;
  if (!ig_shape_ok(args->n, args->slabs)) return DAD_E_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const bool f16 = args->precision == DAD_PREC_FP16;
  const IgWs L = ig_ws_layout(args->precision);
  char* ws = (char*)workspace;

  DAD_TRY(hipMemsetAsync(args->counts, 0, sizeof(int64_t) * DAD_IG_COUNTS, stream));
  if (args->slabs == 0) return DAD_OK;
  IgArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.store = args->store; ia.rows = args->rows; ia.lens = args->lens; ia.slab_off = args->slab_off;
  ia.n = (int)args->n; ia.slabs = (int)args->slabs;
  ia.params = args->params;
  ia.w1h = (const uint16_t*)(ws + L.w1h); ia.w1t = (const uint16_t*)(ws + L.w1t);
  ia.dz = args->dz; ia.delta_in = args->delta_in;
  ia.grad = args->grad; ia.delta_out = args->delta_out; ia.frame_l1 = args->frame_l1;
  ia.counts = (unsigned long long*)args->counts;
  ia.alpha = args->alpha; ia.radius = args->radius;
  if (f16) {
    hipLaunchKernelGGL(dad_ig_w1h, dim3((DAD_H * DAD_D + 255) / 256), dim3(256), 0, stream, args->params,
                       (uint16_t*)(ws + L.w1h), (uint16_t*)(ws + L.w1t));
    DAD_TRY(hipGetLastError());
  }
  switch (dt) {
    case DAD_STORE_F16: launch_slab<DAD_STORE_F16>(ia, f16, stream); break;
    case DAD_STORE_BF16: launch_slab<DAD_STORE_BF16>(ia, f16, stream); break;
    default: launch_slab<DAD_STORE_F32>(ia, f16, stream); break;
  }
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}
