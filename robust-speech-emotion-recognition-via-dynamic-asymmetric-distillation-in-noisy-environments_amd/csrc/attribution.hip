// Exact integrated gradients of a split, store-fed (dad.h, "attributions of a split"): for every utterance of a
// FeatureStore split, a baseline row x' and a caller's logit cotangent dz_u[4] held fixed along the straight path
// x' -> x_t, the attribution of F = dz_u . z to every frame and channel.  The pre-activation is affine in the path
// parameter, so the path integral of ReLU' is the length lambda_tj of the interval on which unit j of frame t is
// active: a closed form, no path sampling.
//
// Launches: a prologue (p0 = W1 x' + b1 and W1 x', 256 values each, one wave per hidden unit in a fixed order; the
// baseline row, zeros when NULL), in FP16 the two fp16 copies of W1, the slab kernel, and a finish kernel (the
// per-utterance sums in slab order).  The slab kernel has dad_input_grad_slab's work unit: one wave = one 32-frame
// slab against all 256 hidden units, four waves per workgroup, rows read in place.  Per slab:
//   forward    a = W1 x with the operands SWAPPED (W1 is the A operand, the rows are B): lane (i, kh) then holds
//              frame i, and accumulator register r = 4 q + e of hidden tile ht holds hidden unit 32 ht + 8 q + 4 kh + e
//              (dad_acc_row).  The k order is eval_rows.h's, the loaders are its Raw4 / Raw8.
//   lambda     per register, in fp32: p1 = p0 + (a - W1 x') (p0 and W1 x' staged in LDS per workgroup, g_u per wave),
//              the four-case closed form, the frame's share sum_j g_j (ReLU p1 - ReLU p0) by one fma per unit in
//              register order, and (FULL) the coefficient lambda g_j written back over the accumulator.
//   backward   (FULL only, a template instance) G = (lambda (.) g_u) W1.  The coefficient of register (ht, 4 q + e)
//              is the (j0 = 32 ht + 8 q, 4 kh + e) element that the fp32 k-step feeds to mfma_f32_32x32x2f32, so it is
//              an A fragment where it was born: no LDS, no ballot.  FP16: the eight halves of k-step (ht, q / 2) are
//              registers 8 (q / 2) .. + 7 of the tile; the B rows come from a transposed W1 copy whose hidden order
//              is permuted to that.  24 column tiles in 3 groups of 8, as dad_input_grad.
//   epilogue   attr = (x - x') G per element in the explicit layout (the stored element is read again, one column tile
//              ahead of its use: with one wave per SIMD nothing else hides that latency), the slab's channel sums
//              to the workspace.
// Counts by one integer atomic per wave and slot.  No floating-point atomics anywhere.
#include <cmath>
#include <cstring>

#include "dad_common.h"
#include "dad_kernels.h"
#include "eval_rows.h"

namespace {

constexpr int kAtThreads = 256;      // 4 waves, one slab each
constexpr int kAtWaves = kAtThreads / 64;
constexpr int kColTiles = DAD_D / 32;             // 24
constexpr int kGroupTiles = 8;                    // column tiles whose accumulators are live together
constexpr int kGroups = kColTiles / kGroupTiles;  // 3
static_assert(kColTiles % kGroupTiles == 0, "column groups");
constexpr int kScaleExp = 14;        // FP16: max |c s| lies in [2^14, 2^15) (dad_input_grad's c_u)
constexpr int kScaleExpMax = 100;
constexpr float kFltMax = 3.402823466e38f;

struct AtArgs {
  const void* store;
  const int64_t* rows; const int32_t* lens; const int32_t* slab_off;
  int n, slabs;
  const float* params;               // flat [W1|b1|W2|b2]
  const uint16_t* w1h;               // FP16: row-major fp16 W1 copy [256][768]
  const uint16_t* w1p;               // FP16, FULL: transposed fp16 W1 copy [768][256], hidden order permuted
  const float* p0;                   // [256] W1 x' + b1
  const float* wb;                   // [256] W1 x'
  const float* xb;                   // [768] x'
  const float* dz;                   // [n][4]
  float* attr; float* frame_attr;
  float* chan_part;                  // [slabs][768] or NULL
  float* slab_tot;                   // [slabs]
  unsigned long long* counts;
};

// position of hidden unit j in the permuted order: k-step s = j / 16 of mfma_f32_32x32x16_f16 takes from lane
// (i, kh) the halves jj = 0 .. 7 at k = 8 kh + jj, and that lane's registers are the units 16 s + 8 (jj / 4) + 4 kh +
// jj % 4
__device__ __forceinline__ int at_perm_pos(int j) {
  const int w = j & 15;
  return (j & ~15) + 8 * ((w >> 2) & 1) + 4 * ((w >> 3) & 1) + (w & 3);
}

// fp16 copies of W1: row-major for the forward, transposed and permuted for the data-gradient GEMM (wp may be NULL)
__global__ __launch_bounds__(256) void dad_at_w1h(const float* params, uint16_t* w, uint16_t* wp) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)DAD_H * DAD_D) return;
  const uint16_t h = dad_half_bits(params[DAD_OFF_W1 + e], true);
  const size_t j = e / DAD_D, d = e % DAD_D;
  w[e] = h;
  if (wp) wp[d * DAD_H + at_perm_pos((int)j)] = h;
}

// One wave per hidden unit j: wb[j] = W1[j] . x' (lane l: channels l, l + 64, ... by fmas, then a fixed xor tree),
// p0[j] = wb[j] + b1[j].  FP16: both operands rounded to fp16 first, as the GEMM sees them.  Block 0 also writes the
// baseline row (zeros when NULL).
template <bool F16>
__global__ __launch_bounds__(256) void dad_at_prologue(const float* params, const float* baseline, float* p0,
                                                       float* wb, float* xb) {
  DAD_GUARD_BLOCK(256);
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0)
    for (int d = threadIdx.x; d < DAD_D; d += 256) xb[d] = baseline ? baseline[d] : 0.0f;
  if (j >= DAD_H) return;
  const float* w = params + DAD_OFF_W1 + (size_t)j * DAD_D;
  float s = 0.0f;
  for (int d = lane; d < DAD_D; d += 64) {
    float wv = w[d], xv = baseline ? baseline[d] : 0.0f;
    if constexpr (F16) { wv = (float)(_Float16)wv; xv = (float)(_Float16)xv; }
    s = fmaf(wv, xv, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) {
    wb[j] = s;
    p0[j] = s + params[DAD_OFF_B1 + j];
  }
}

// one element of a store row, widened to f32 (the value Raw4::get gives)
template <int DT>
__device__ __forceinline__ float at_store_elem(const void* store, uint32_t el) {
  if constexpr (DT == DAD_STORE_F32) return ((const float*)store)[el];
  else if constexpr (DT == DAD_STORE_F16) return Raw4<DAD_STORE_F16>::h(((const uint16_t*)store)[el]);
  else return __uint_as_float((uint32_t)((const uint16_t*)store)[el] << 16);
}

// eval_slab_f32's pipeline and k order for one network with the MFMA operands swapped: acc[ht] register r of lane
// (i, kh) = sum_d W1[32 ht + dad_acc_row(r, kh)][d] x_i[d]
template <int DT>
__device__ __forceinline__ void at_forward_f32(const void* store, size_t xel, const float* W, f32x16 (&acc)[DAD_HT]) {
  Raw4<DT> xc, xn;
  f32x4 wc[DAD_HT], wn[DAD_HT];
  xc.load(store, xel);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 8) {
    const int dn = d0 + 8 < DAD_D ? d0 + 8 : d0;   // the last step reloads itself
    xn.load(store, xel + dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D + dn);
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 x = xc.get();
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[ht][e], x[e], acc[ht], 0, 0, 0);
    xc = xn;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// eval_slab_f16's, swapped likewise
template <int DT>
__device__ __forceinline__ void at_forward_f16(const void* store, size_t xel, const uint16_t* W,
                                               f32x16 (&acc)[DAD_HT]) {
  Raw8<DT> xc, xn;
  u32x4 wc[DAD_HT], wn[DAD_HT];
  xc.load(store, xel);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 16) {
    const int dn = d0 + 16 < DAD_D ? d0 + 16 : d0;
    xn.load(store, xel + dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D + dn);
    __builtin_amdgcn_sched_barrier(0);
    const f16x8 x = __builtin_bit_cast(f16x8, xc.frag());
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
      acc[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wc[ht]), x, acc[ht], 0, 0, 0);
    xc = xn;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

template <int DT, bool F16, bool FULL>
__global__ __launch_bounds__(kAtThreads) void dad_attribution_slab(AtArgs a) {
  DAD_GUARD_BLOCK(kAtThreads);
  // g_u as floats; FP16 FULL: c_u s_u as floats behind it
  __shared__ __attribute__((aligned(16))) float s_g[kAtWaves][(F16 && FULL) ? 2 * DAD_H : DAD_H];
  __shared__ __attribute__((aligned(16))) float s_p0[DAD_H], s_wb[DAD_H];      // the call's p0 and W1 x'
  s_p0[threadIdx.x] = a.p0[threadIdx.x];
  s_wb[threadIdx.x] = a.wb[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kAtWaves + wv));
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
    for (int d = lane; d < DAD_D; d += 64) {
      if (a.attr)
        for (int r = 0; r < DAD_SLAB; ++r) a.attr[(out0 + r) * DAD_D + d] = 0.0f;
      if (a.chan_part) a.chan_part[(size_t)job * DAD_D + d] = 0.0f;
    }
    if (a.frame_attr && lane < DAD_SLAB) a.frame_attr[out0 + lane] = 0.0f;
    if (lane == 0) a.slab_tot[job] = 0.0f;
    return;
  }
  float* gl = s_g[wv];
  const float lenf = fmaxf((float)len, 1.0f);

  // ---- g_u (dad_input_grad's order) -----------------------------------------------------------------------
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
#pragma unroll
    for (int e = 0; e < 4; ++e) gl[4 * lane + e] = s[e] / lenf;
    if constexpr (F16 && FULL) {
      float m = fmaxf(fmaxf(fabsf(s[0]), fabsf(s[1])), fmaxf(fabsf(s[2]), fabsf(s[3])));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      int ex = 0;
      if (m > 0.0f && m <= kFltMax) ex = min(kScaleExp - ilogbf(m), kScaleExpMax);
      const float cu = ldexpf(1.0f, ex);
      invc = ldexpf(1.0f, -ex);
#pragma unroll
      for (int e = 0; e < 4; ++e) gl[DAD_H + 4 * lane + e] = s[e] * cu;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- forward GEMM, operands swapped: lane (i, kh) holds frame i ---------------------------------------------
  f32x16 acc[DAD_HT];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) acc[ht] = f32x16{};
  const int64_t row0 = a.rows[u] + (int64_t)c * DAD_SLAB;
  const int lastv = len - 1 - c * DAD_SLAB;        // the slab's last valid row (>= 0 here)
  {
    // past the last frame: the utterance's last frame again (its coefficients are selected to 0 below)
    const size_t row = (size_t)(row0 + (int64_t)min(i, lastv));
    if constexpr (F16) at_forward_f16<DT>(a.store, row * DAD_D + 8 * kh, a.w1h + (size_t)i * DAD_D + 8 * kh, acc);
    else at_forward_f32<DT>(a.store, row * DAD_D + 4 * kh, a.params + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh, acc);
  }

  // ---- lambda, the frame's share, the coefficients ---------------------------------------------------------
  const bool rowv = (vbits >> i) & 1u;
  float fs = 0.0f;
  unsigned int n_cross = 0u, n_one = 0u;
  uint32_t cf[FULL && F16 ? DAD_HT : 1][8];        // FP16: the packed coefficients of a tile
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    __builtin_amdgcn_sched_barrier(0);               // one tile's LDS reads in flight, not all eight
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 32 * ht + 8 * q + 4 * kh;
      const f32x4 p0v = *reinterpret_cast<const f32x4*>(s_p0 + j);
      const f32x4 wbv = *reinterpret_cast<const f32x4*>(s_wb + j);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gl + j);
      f32x4 gc = gv;
      if constexpr (F16 && FULL) gc = *reinterpret_cast<const f32x4*>(gl + DAD_H + j);
      float co[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p0 = p0v[e];
        const float p1 = p0 + (acc[ht][4 * q + e] - wbv[e]);
        const float r1 = !(p1 <= 0.0f) ? p1 : 0.0f;     // ReLU that keeps a NaN
        const float r0 = p0 > 0.0f ? p0 : 0.0f;
        fs = fmaf(gv[e], r1 - r0, fs);
        const bool pos0 = p0 > 0.0f, pos1 = p1 > 0.0f;
        // one division whatever the case (no divergent branch): p1 / (p1 - p0) or p0 / (p0 - p1) on a crossing
        float qd = (pos1 ? p1 : p0) / (pos1 ? p1 - p0 : p0 - p1);
        asm("" : "+v"(qd));       // keeps the quotient out of the select, which would else become a branch around it
        float lam = pos0 != pos1 ? qd : (pos0 ? 1.0f : 0.0f);
        lam = p1 != p1 ? p1 : lam;
        n_cross += (rowv && pos0 != pos1) ? 1u : 0u;
        n_one += (rowv && pos0 && pos1) ? 1u : 0u;
        co[e] = rowv ? lam * gc[e] : 0.0f;             // selection, no product with 0
      }
      if constexpr (FULL) {
        if constexpr (F16) {
          cf[ht][2 * q] = dad_pack2<true>(co[0], co[1]);
          cf[ht][2 * q + 1] = dad_pack2<true>(co[2], co[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ht][4 * q + e] = co[e];
        }
      }
    }
  }
  {
    fs += __shfl_xor(fs, 32, 64);                      // the other half of the hidden units
    float st = rowv ? fs : 0.0f;
    if (a.frame_attr && kh == 0) a.frame_attr[out0 + i] = st;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) st += __shfl_xor(st, o, 64);
    if (lane == 0) a.slab_tot[job] = st;
  }
  unsigned int n_bad = 0u;

  // ---- data-gradient GEMM in column groups, and the epilogue ----------------------------------------------
  if constexpr (FULL) {
    const size_t esz = DT == DAD_STORE_F32 ? 4 : 2;
    const void* xslab = (const char*)a.store + (size_t)row0 * DAD_D * esz;
    float* aslab = a.attr ? a.attr + out0 * DAD_D : nullptr;
#pragma unroll 1
    for (int g = 0; g < kGroups; ++g) {
      const int d0 = g * kGroupTiles * 32;
      f32x16 ac2[kGroupTiles];
#pragma unroll
      for (int ct = 0; ct < kGroupTiles; ++ct) ac2[ct] = f32x16{};
      if constexpr (F16) {
        // k-step s = 2 ht + qp: B = W1P[d0 + 32 ct + i][16 s + 8 kh ..]
        const uint16_t* B = a.w1p + (size_t)(d0 + i) * DAD_H + 8 * kh;
        u32x4 bc[kGroupTiles], bn[kGroupTiles];
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct) bc[ct] = *reinterpret_cast<const u32x4*>(B + (size_t)ct * 32 * DAD_H);
#pragma unroll
        for (int s = 0; s < DAD_H / 16; ++s) {
          const int sn = s + 1 < DAD_H / 16 ? s + 1 : s;   // the last step reloads itself
#pragma unroll
          for (int ct = 0; ct < kGroupTiles; ++ct)
            bn[ct] = *reinterpret_cast<const u32x4*>(B + (size_t)ct * 32 * DAD_H + 16 * sn);
          const int ht = s >> 1, qp = s & 1;
          const u32x4 hv = u32x4{cf[ht][4 * qp], cf[ht][4 * qp + 1], cf[ht][4 * qp + 2], cf[ht][4 * qp + 3]};
          __builtin_amdgcn_sched_barrier(0);
          const f16x8 av = __builtin_bit_cast(f16x8, hv);
#pragma unroll
          for (int ct = 0; ct < kGroupTiles; ++ct)
            ac2[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, __builtin_bit_cast(f16x8, bc[ct]), ac2[ct], 0, 0, 0);
#pragma unroll
          for (int ct = 0; ct < kGroupTiles; ++ct) bc[ct] = bn[ct];
        }
      } else {
        // k-step (j0 = 8 ks, e, kh): hidden unit j0 + 4 kh + e; B = W1[that unit][d0 + 32 ct + i]
        const float* B = a.params + DAD_OFF_W1 + (size_t)(4 * kh) * DAD_D + d0 + i;
        float bc[kGroupTiles][4], bn[kGroupTiles][4];
#pragma unroll
        for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) bc[ct][e] = B[(size_t)e * DAD_D + ct * 32];
#pragma unroll
        for (int ks = 0; ks < DAD_H / 8; ++ks) {
          const int jn = ks + 1 < DAD_H / 8 ? 8 * (ks + 1) : 8 * ks;   // the last step reloads itself
#pragma unroll
          for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) bn[ct][e] = B[(size_t)(jn + e) * DAD_D + ct * 32];
          const int ht = ks >> 2, q = ks & 3;
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              ac2[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[ht][4 * q + e], bc[ct][e], ac2[ct], 0, 0, 0);
#pragma unroll
          for (int ct = 0; ct < kGroupTiles; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) bc[ct][e] = bn[ct][e];
        }
      }
      // lane (i, kh) of register r holds G[row dad_acc_row(r, kh)][d0 + 32 ct + i].  The slab's rows and its
      // block of attr are addressed by 32-bit offsets from wave-uniform bases.
      // the next tile's sixteen row elements are fetched while this tile's are used
      float xv[2][16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        xv[0][r] = at_store_elem<DT>(xslab, (uint32_t)(min(dad_acc_row(r, kh), lastv) * DAD_D + d0 + i));
#pragma unroll
      for (int ct = 0; ct < kGroupTiles; ++ct) {
        __builtin_amdgcn_sched_barrier(0);
        const int d = d0 + ct * 32 + i;
        if (ct + 1 < kGroupTiles) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            xv[(ct + 1) & 1][r] = at_store_elem<DT>(xslab, (uint32_t)(min(dad_acc_row(r, kh), lastv) * DAD_D + d + 32));
        }
        const float xb = a.xb[d];
        float cs = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rw = dad_acc_row(r, kh);
          const bool v = (vbits >> rw) & 1u;
          const float x = xv[ct & 1][r];
          float G = ac2[ct][r];
          if constexpr (F16) G = (G * invc) / lenf;
          float at = (x - xb) * G;
          const bool fin = fabsf(at) <= kFltMax;
          n_bad += (v && !fin) ? 1u : 0u;
          at = (v && fin) ? at : 0.0f;
          cs += at;
          if (a.attr) aslab[(uint32_t)(rw * DAD_D + d)] = at;
        }
        cs += __shfl_xor(cs, 32, 64);                  // the other sixteen rows
        if (a.chan_part && kh == 0) a.chan_part[(size_t)job * DAD_D + d] = cs;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_bad += __shfl_xor(n_bad, o, 64);
    n_cross += __shfl_xor(n_cross, o, 64);
    n_one += __shfl_xor(n_one, o, 64);
  }
  if (lane == 0) {
    atomicAdd(a.counts + DAD_AT_FRAMES, (unsigned long long)__popc(vbits));
    if (n_bad) atomicAdd(a.counts + DAD_AT_NONFINITE, (unsigned long long)n_bad);
    if (n_cross) atomicAdd(a.counts + DAD_AT_CROSS, (unsigned long long)n_cross);
    if (n_one) atomicAdd(a.counts + DAD_AT_ONE, (unsigned long long)n_one);
  }
}

// One workgroup per utterance: chan_attr[u][d] = the slab partials in slab order; utt_total[u] = the slab totals,
// lane l of wave 0 taking slabs l, l + 64, ... in order, then a fixed xor tree.  An utterance that owns no slab gets
// zeros.
__global__ __launch_bounds__(256) void dad_at_finish(const int32_t* slab_off, int slabs, const float* chan_part,
                                                     const float* slab_tot, float* chan_attr, float* utt_total) {
  DAD_GUARD_BLOCK(256);
  const size_t u = blockIdx.x;
  const int s0 = max(slab_off[u], 0), s1 = min(slab_off[u + 1], slabs);
  if (chan_attr) {
    for (int d = threadIdx.x; d < DAD_D; d += 256) {
      float s = 0.0f;
      for (int k = s0; k < s1; ++k) s += chan_part[(size_t)k * DAD_D + d];
      chan_attr[u * DAD_D + d] = s;
    }
  }
  if (utt_total && threadIdx.x < 64) {
    float s = 0.0f;
    for (int k = s0 + (int)threadIdx.x; k < s1; k += 64) s += slab_tot[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) utt_total[u] = s;
  }
}

// The frame-only pieces first, so that the bytes a frame-only call touches are a prefix of the full layout.
struct AtWs {
  size_t p0, wb, xb, w1h, slab_tot, frame_bytes, w1p, chan_part, bytes;
};

AtWs at_ws_layout(int64_t slabs, int precision) {
  AtWs w;
  size_t off = 0;
  const size_t wbytes = precision == DAD_PREC_FP16 ? sizeof(uint16_t) * DAD_H * DAD_D : 0;
  w.p0 = off; off = dad_align(off + sizeof(float) * DAD_H);
  w.wb = off; off = dad_align(off + sizeof(float) * DAD_H);
  w.xb = off; off = dad_align(off + sizeof(float) * DAD_D);
  w.w1h = off; off = dad_align(off + wbytes);
  w.slab_tot = off; off = dad_align(off + sizeof(float) * (size_t)slabs);
  w.frame_bytes = off;
  w.w1p = off; off = dad_align(off + wbytes);
  w.chan_part = off; off = dad_align(off + sizeof(float) * (size_t)slabs * DAD_D);
  w.bytes = off;
  return w;
}

bool at_shape_ok(int64_t n, int64_t slabs) {
  return n >= 1 && n <= 0x7fffffffLL && slabs >= 0 && slabs <= n * (int64_t)(1 << 26) && slabs <= 0x7fffffffLL;
}

int at_check(const dad_attribution_args* args) {
  if (!args) return DAD_E_ARG;
  if (!args->store || !args->rows || !args->lens || !args->slab_off || !args->params || !args->dz || !args->counts)
    return DAD_E_ARG;
  const int dt = args->store_dtype;
  if (dt != DAD_STORE_F32 && dt != DAD_STORE_F16 && dt != DAD_STORE_BF16) return DAD_E_ARG;
  if (args->precision == DAD_PREC_BF16) return DAD_E_UNSUPPORTED;
  if (args->precision != DAD_PREC_FP32 && args->precision != DAD_PREC_FP16) return DAD_E_ARG;
  if (!at_shape_ok(args->n, args->slabs)) return DAD_E_SHAPE;
  return DAD_OK;
}

template <int DT>
void launch_slab(const AtArgs& aa, bool f16, bool full, hipStream_t stream) {
  const dim3 grid((unsigned)((aa.slabs + kAtWaves - 1) / kAtWaves)), block(kAtThreads);
  if (f16) {
    if (full) hipLaunchKernelGGL((dad_attribution_slab<DT, true, true>), grid, block, 0, stream, aa);
    else hipLaunchKernelGGL((dad_attribution_slab<DT, true, false>), grid, block, 0, stream, aa);
  } else {
    if (full) hipLaunchKernelGGL((dad_attribution_slab<DT, false, true>), grid, block, 0, stream, aa);
    else hipLaunchKernelGGL((dad_attribution_slab<DT, false, false>), grid, block, 0, stream, aa);
  }
}

}  // namespace

extern "C" size_t dad_attribution_workspace_bytes(int64_t n, int64_t slabs, int precision) {
  if (!at_shape_ok(n, slabs)) return 0;
  return at_ws_layout(slabs, precision).bytes;
}

extern "C" int dad_attribution_plan(const dad_attribution_args* args, int64_t* out) {
  if (!out) return DAD_E_ARG;
  const int rc = at_check(args);
  if (rc != DAD_OK) return rc;
  const bool full = args->attr || args->chan_attr;
  const bool f16 = args->precision == DAD_PREC_FP16;
  const AtWs L = at_ws_layout(args->slabs, args->precision);
  out[DAD_AT_PLAN_MODE] = full ? 1 : 0;
  out[DAD_AT_PLAN_BYTES] = (int64_t)(!full ? L.frame_bytes : args->chan_attr ? L.bytes : L.chan_part);
  const bool finish = args->chan_attr || args->utt_total;
  out[DAD_AT_PLAN_LAUNCHES] = args->slabs == 0 ? (finish ? 1 : 0) : 2 + (f16 ? 1 : 0) + (finish ? 1 : 0);
  out[DAD_AT_PLAN_KERNEL] = 4 * args->store_dtype + 2 * (f16 ? 1 : 0) + (full ? 1 : 0);
  return DAD_OK;
}

extern "C" int dad_attribution(const dad_attribution_args* args, void* workspace, void* stream_) {
  if (!args || !workspace) return DAD_E_ARG;
  const int rc = at_check(args);
  if (rc != DAD_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int dt = args->store_dtype;
  const bool f16 = args->precision == DAD_PREC_FP16;
  const bool full = args->attr || args->chan_attr;
  const AtWs L = at_ws_layout(args->slabs, args->precision);
  char* ws = (char*)workspace;

  DAD_TRY(hipMemsetAsync(args->counts, 0, sizeof(int64_t) * DAD_AT_COUNTS, stream));
  if (args->slabs > 0) {
    AtArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.store = args->store; aa.rows = args->rows; aa.lens = args->lens; aa.slab_off = args->slab_off;
    aa.n = (int)args->n; aa.slabs = (int)args->slabs;
    aa.params = args->params;
    aa.w1h = (const uint16_t*)(ws + L.w1h); aa.w1p = (const uint16_t*)(ws + L.w1p);
    aa.p0 = (const float*)(ws + L.p0); aa.wb = (const float*)(ws + L.wb); aa.xb = (const float*)(ws + L.xb);
    aa.dz = args->dz;
    aa.attr = args->attr; aa.frame_attr = args->frame_attr;
    aa.chan_part = args->chan_attr ? (float*)(ws + L.chan_part) : nullptr;
    aa.slab_tot = (float*)(ws + L.slab_tot);
    aa.counts = (unsigned long long*)args->counts;
    if (f16) {
      hipLaunchKernelGGL(dad_at_prologue<true>, dim3(DAD_H / 4), dim3(256), 0, stream, args->params, args->baseline,
                         (float*)(ws + L.p0), (float*)(ws + L.wb), (float*)(ws + L.xb));
      hipLaunchKernelGGL(dad_at_w1h, dim3((DAD_H * DAD_D + 255) / 256), dim3(256), 0, stream, args->params,
                         (uint16_t*)(ws + L.w1h), full ? (uint16_t*)(ws + L.w1p) : (uint16_t*)nullptr);
    } else {
      hipLaunchKernelGGL(dad_at_prologue<false>, dim3(DAD_H / 4), dim3(256), 0, stream, args->params, args->baseline,
                         (float*)(ws + L.p0), (float*)(ws + L.wb), (float*)(ws + L.xb));
    }
    DAD_TRY(hipGetLastError());
    switch (dt) {
      case DAD_STORE_F16: launch_slab<DAD_STORE_F16>(aa, f16, full, stream); break;
      case DAD_STORE_BF16: launch_slab<DAD_STORE_BF16>(aa, f16, full, stream); break;
      default: launch_slab<DAD_STORE_F32>(aa, f16, full, stream); break;
    }
    DAD_TRY(hipGetLastError());
  }
  if (args->chan_attr || args->utt_total) {
    hipLaunchKernelGGL(dad_at_finish, dim3((unsigned)args->n), dim3(256), 0, stream, args->slab_off, (int)args->slabs,
                       (const float*)(ws + L.chan_part), (const float*)(ws + L.slab_tot), args->chan_attr,
                       args->utt_total);
    DAD_TRY(hipGetLastError());
  }
  return DAD_OK;
}
