// What the store-fed evaluators share (eval_split.hip: one embedding per utterance; eval_windows.hip: one per
// window of an utterance; eval_noise.hip: one per noise level of an utterance): the in-place row loaders of the
// three store types, one slab's GEMM loop in both operand precisions (and with additive noise as a second operand),
// the slab epilogue (bias, ReLU, masked row sum) and the head arithmetic behind a pooled embedding.  Everything is
// internal to the including unit.
#ifndef DAD_EVAL_ROWS_H_
#define DAD_EVAL_ROWS_H_

#include "dad_common.h"
#include "dad_kernels.h"

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---- store rows: 4 (fp32 path) or 8 (fp16 path) consecutive channels of one row ---------------
template <int DT> struct Raw4;
template <> struct Raw4<DAD_STORE_F32> {
  f32x4 v;
  __device__ __forceinline__ void load(const void* base, size_t el) { v = *reinterpret_cast<const f32x4*>((const float*)base + el); }
  __device__ __forceinline__ f32x4 get() const { return v; }
};
// halves one scalar at a time, as collate.hip widens them
template <> struct Raw4<DAD_STORE_F16> {
  u32x2 v;
  __device__ __forceinline__ void load(const void* base, size_t el) { v = *reinterpret_cast<const u32x2*>((const uint16_t*)base + el); }
  static __device__ __forceinline__ float h(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
  __device__ __forceinline__ f32x4 get() const {
    f32x4 r;
    r[0] = h(v[0] & 0xffffu); r[1] = h(v[0] >> 16); r[2] = h(v[1] & 0xffffu); r[3] = h(v[1] >> 16);
    return r;
  }
};
template <> struct Raw4<DAD_STORE_BF16> {
  u32x2 v;
  __device__ __forceinline__ void load(const void* base, size_t el) { v = *reinterpret_cast<const u32x2*>((const uint16_t*)base + el); }
  __device__ __forceinline__ f32x4 get() const {
    f32x4 r;
    r[0] = __uint_as_float(v[0] << 16); r[1] = __uint_as_float(v[0] & 0xffff0000u);
    r[2] = __uint_as_float(v[1] << 16); r[3] = __uint_as_float(v[1] & 0xffff0000u);
    return r;
  }
};

// 8 channels as the packed fp16 A fragment of one 32x32x16 k-step
template <int DT> struct Raw8;
template <> struct Raw8<DAD_STORE_F32> {
  f32x4 a, b;
  __device__ __forceinline__ void load(const void* base, size_t el) {
    const f32x4* p = reinterpret_cast<const f32x4*>((const float*)base + el);
    a = p[0]; b = p[1];
  }
  __device__ __forceinline__ u32x4 frag() const {
    return u32x4{dad_pack2<true>(a[0], a[1]), dad_pack2<true>(a[2], a[3]), dad_pack2<true>(b[0], b[1]),
                 dad_pack2<true>(b[2], b[3])};
  }
};
template <> struct Raw8<DAD_STORE_F16> {   // already fp16: widening then rounding back is the identity
  u32x4 v;
  __device__ __forceinline__ void load(const void* base, size_t el) { v = *reinterpret_cast<const u32x4*>((const uint16_t*)base + el); }
  __device__ __forceinline__ u32x4 frag() const { return v; }
};
template <> struct Raw8<DAD_STORE_BF16> {
  u32x4 v;
  __device__ __forceinline__ void load(const void* base, size_t el) { v = *reinterpret_cast<const u32x4*>((const uint16_t*)base + el); }
  __device__ __forceinline__ u32x4 frag() const {
    u32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      r[k] = dad_pack2<true>(__uint_as_float(v[k] << 16), __uint_as_float(v[k] & 0xffff0000u));
    return r;
  }
};

// owner of job `job` under an exclusive prefix off[n + 1]: the largest u in [0, n) with off[u] <= job (an
// utterance that owns no job is never the answer)
__device__ __forceinline__ int slab_owner(const int32_t* slab_off, int n, int job) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slab_off[mid] <= job) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// bias + ReLU + sum over the slab's rows whose bit is set in vbits (the part_sum half of dad_encode_f32's
// epilogue)
__device__ __forceinline__ void eval_epilogue(const f32x16* acc, const float* bias, float* part, uint32_t vbits) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 31, kh = lane >> 5;
  float bhs[DAD_HT];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) bhs[ht] = bias[ht * 32 + j];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool v = (vbits >> dad_acc_row(r, kh)) & 1u;
      const float pre = acc[ht][r] + bhs[ht];
      s += (v && !(pre <= 0.0f)) ? pre : 0.0f;   // ReLU that keeps a NaN (torch's), so bad features show
    }
    s += __shfl_xor(s, 32, 64);
    if (kh == 0) part[ht * 32 + j] = s;
  }
}

// FP32: k-step (d0, e, kh) uses channel d0 + 4 kh + e of both operands; the next step's x chunk and
// W1 fragments are loaded while this step's MFMAs run (dad_encode_f32's pipeline).
template <int DT, bool TEACH>
__device__ __forceinline__ void eval_slab_f32(const void* store, size_t xel, const float* Ws, const float* Wt,
                                              f32x16 (&acc0)[DAD_HT], f32x16 (&acc1)[DAD_HT]) {
  constexpr int NW = TEACH ? 2 : 1;
  Raw4<DT> xc, xn;
  f32x4 wc[NW][DAD_HT], wn[NW][DAD_HT];
  xc.load(store, xel);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    wc[0][ht] = *reinterpret_cast<const f32x4*>(Ws + (size_t)ht * 32 * DAD_D);
    if constexpr (TEACH) wc[1][ht] = *reinterpret_cast<const f32x4*>(Wt + (size_t)ht * 32 * DAD_D);
  }
  for (int d0 = 0; d0 < DAD_D; d0 += 8) {
    const int dn = d0 + 8 < DAD_D ? d0 + 8 : d0;   // the last step reloads itself
    xn.load(store, xel + dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) {
      wn[0][ht] = *reinterpret_cast<const f32x4*>(Ws + (size_t)ht * 32 * DAD_D + dn);
      if constexpr (TEACH) wn[1][ht] = *reinterpret_cast<const f32x4*>(Wt + (size_t)ht * 32 * DAD_D + dn);
    }
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 x = xc.get();
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], wc[0][ht][e], acc0[ht], 0, 0, 0);
        if constexpr (TEACH) acc1[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], wc[1][ht][e], acc1[ht], 0, 0, 0);
      }
    xc = xn;
#pragma unroll
    for (int k = 0; k < NW; ++k)
#pragma unroll
      for (int ht = 0; ht < DAD_HT; ++ht) wc[k][ht] = wn[k][ht];
  }
}

// FP16: 32x32x16 k-steps; lane (i, kh) holds A[row i][k = 8 kh + j] and B[k = 8 kh + j][h = i]
template <int DT, bool TEACH>
__device__ __forceinline__ void eval_slab_f16(const void* store, size_t xel, const uint16_t* Ws, const uint16_t* Wt,
                                              f32x16 (&acc0)[DAD_HT], f32x16 (&acc1)[DAD_HT]) {
  constexpr int NW = TEACH ? 2 : 1;
  Raw8<DT> xc, xn;
  u32x4 wc[NW][DAD_HT], wn[NW][DAD_HT];
  xc.load(store, xel);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    wc[0][ht] = *reinterpret_cast<const u32x4*>(Ws + (size_t)ht * 32 * DAD_D);
    if constexpr (TEACH) wc[1][ht] = *reinterpret_cast<const u32x4*>(Wt + (size_t)ht * 32 * DAD_D);
  }
  for (int d0 = 0; d0 < DAD_D; d0 += 16) {
    const int dn = d0 + 16 < DAD_D ? d0 + 16 : d0;
    xn.load(store, xel + dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) {
      wn[0][ht] = *reinterpret_cast<const u32x4*>(Ws + (size_t)ht * 32 * DAD_D + dn);
      if constexpr (TEACH) wn[1][ht] = *reinterpret_cast<const u32x4*>(Wt + (size_t)ht * 32 * DAD_D + dn);
    }
    __builtin_amdgcn_sched_barrier(0);
    const f16x8 x = __builtin_bit_cast(f16x8, xc.frag());
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) {
      acc0[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, wc[0][ht]), acc0[ht], 0, 0, 0);
      if constexpr (TEACH)
        acc1[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, wc[1][ht]), acc1[ht], 0, 0, 0);
    }
    xc = xn;
#pragma unroll
    for (int k = 0; k < NW; ++k)
#pragma unroll
      for (int ht = 0; ht < DAD_HT; ++ht) wc[k][ht] = wn[k][ht];
  }
}

// One network's head behind a pooled sum (dad_predict_head_kernel's arithmetic): lane l holds the sum's
// components 4 l .. 4 l + 3 in s; the embedding is s / max(len, 1).  Output row u.  Returns the first-maximum
// argmax; *bad = a logit is not finite.  Lane 0 writes the outputs.  hv receives what a caller that compares two
// heads needs: the lane's embedding components, the logits, their maximum, sum exp(z - m) and the probabilities
// (the same in every lane).
struct HeadVals {
  f32x4 x;
  float z[DAD_C], p[DAD_C];
  float m, se;
};
__device__ __forceinline__ int eval_head_pooled_v(f32x4 s, float len, const float* flat, int use_entropy, size_t u,
                                                  float* emb, float* logits, float* probs, float* score_out,
                                                  float* score_ws, bool* bad, HeadVals& hv) {
  const int lane = threadIdx.x & 63;
  const float d = fmaxf(len, 1.0f);
  f32x4 x;
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = s[e] / d;
  if (emb) *reinterpret_cast<f32x4*>(emb + u * DAD_H + 4 * lane) = x;
  const float* w2 = flat + DAD_OFF_W2;
  const float* b2 = flat + DAD_OFF_B2;
  float z[DAD_C];
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(w2 + (size_t)c * DAD_H + 4 * lane);
    float p = x[0] * w[0];
    p = fmaf(x[1], w[1], p);
    p = fmaf(x[2], w[2], p);
    p = fmaf(x[3], w[3], p);
    z[c] = dad_wave_sum(p) + b2[c];
  }
  float m = z[0];
  int am = 0;
  bool nf = !(fabsf(z[0]) <= 3.402823466e38f);
#pragma unroll
  for (int c = 1; c < DAD_C; ++c) {
    if (z[c] > m) { m = z[c]; am = c; }
    nf = nf || !(fabsf(z[c]) <= 3.402823466e38f);
  }
  *bad = nf;
  float ex[DAD_C], se = 0.0f;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) { ex[c] = expf(z[c] - m); se += ex[c]; }
  float p[DAD_C], pmax = 0.0f, ent = 0.0f;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    p[c] = ex[c] / se;
    pmax = fmaxf(pmax, p[c]);
    ent -= p[c] * log2f(p[c] + 1e-8f);            // I/utils.py:417
  }
  if (lane == 0) {
    const float sc = use_entropy ? pmax * (1.0f - ent / 2.0f) : pmax;
    if (logits) {
#pragma unroll
      for (int c = 0; c < DAD_C; ++c) logits[u * DAD_C + c] = z[c];
    }
    if (probs) {
#pragma unroll
      for (int c = 0; c < DAD_C; ++c) probs[u * DAD_C + c] = p[c];
    }
    if (score_out) score_out[u] = sc;
    if (score_ws) score_ws[u] = sc;
  }
  hv.x = x;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) { hv.z[c] = z[c]; hv.p[c] = p[c]; }
  hv.m = m; hv.se = se;
  return am;
}
__device__ __forceinline__ int eval_head_pooled(f32x4 s, float len, const float* flat, int use_entropy, size_t u,
                                                float* emb, float* logits, float* probs, float* score_out,
                                                float* score_ws, bool* bad) {
  HeadVals hv;
  return eval_head_pooled_v(s, len, flat, use_entropy, u, emb, logits, probs, score_out, score_ws, bad, hv);
}

// ---- additive noise on the rows (eval_noise.hip) -----------------------------------------------------------
// The standard normal of (utterance u, frame t, channel d) under stream key skey: a pure function of those four.
// The key is per utterance (and per block of 2^22 frames of it, so the pair index below never wraps in 32 bits:
// 2^22 * 384 < 2^32); element (t mod 2^22) * 768 + d of that key's stream, in dad_normal_pair's pairing.
constexpr int kNoiseFrameBits = 22;
__device__ __forceinline__ uint32_t noise_key(uint32_t skey, int u, int t) {
  const uint32_t ukey = dad_rng32((uint32_t)u, skey);
  const uint32_t hi = (uint32_t)t >> kNoiseFrameBits;
  return hi ? dad_rng32(hi, ukey) : ukey;
}
// pair index of channels d, d + 1 (d even) of frame t
__device__ __forceinline__ uint32_t noise_pair(int t, int d) {
  return ((uint32_t)t & ((1u << kNoiseFrameBits) - 1u)) * (uint32_t)(DAD_D / 2) + ((uint32_t)d >> 1);
}
// channels d .. d + 3 (d % 4 == 0) of the frame whose channel-0 pair is pair0
__device__ __forceinline__ f32x4 noise_normal4(uint32_t key, uint32_t pair0, int d) {
  f32x4 z;
  float a, b, c, e;
  dad_normal_pair(key, pair0 + ((uint32_t)d >> 1), a, b);
  dad_normal_pair(key, pair0 + ((uint32_t)d >> 1) + 1u, c, e);
  z[0] = a; z[1] = b; z[2] = c; z[3] = e;
  return z;
}

// The noise operand of one lane's row: EXPL reads it from an explicit [rows][768] f32 array (element nel is the
// lane's first channel), otherwise it is generated in registers (key, pair0 = noise_pair(t, lane's first channel)).
struct NoiseSrc {
  const float* noise; size_t nel;
  uint32_t key, pair0;
};
template <bool EXPL>
__device__ __forceinline__ f32x4 noise_load4(const NoiseSrc& n, int d) {
  if constexpr (EXPL) return *reinterpret_cast<const f32x4*>(n.noise + n.nel + d);
  else return noise_normal4(n.key, n.pair0, d);
}
// 8 channels as the packed fp16 A fragment of one 32x32x16 k-step
template <bool EXPL>
__device__ __forceinline__ u32x4 noise_frag8(const NoiseSrc& n, int d) {
  const f32x4 a = noise_load4<EXPL>(n, d), b = noise_load4<EXPL>(n, d + 4);
  return u32x4{dad_pack2<true>(a[0], a[1]), dad_pack2<true>(a[2], a[3]), dad_pack2<true>(b[0], b[1]),
               dad_pack2<true>(b[2], b[3])};
}

// eval_slab_f32 with a second A operand on the same W fragment: acc0 += x W1, acc1 += n W1 (the k order of both
// is eval_slab_f32's, so acc0 holds the same bits).  The next step's rows, noise and W1 are fetched while this
// step's MFMAs run.
template <int DT, bool EXPL>
__device__ __forceinline__ void eval_slab_noise_f32(const void* store, size_t xel, const NoiseSrc& nz, const float* W,
                                                    f32x16 (&acc0)[DAD_HT], f32x16 (&acc1)[DAD_HT]) {
  Raw4<DT> xc, xn;
  f32x4 nc, nn;
  f32x4 wc[DAD_HT], wn[DAD_HT];
  xc.load(store, xel);
  nc = noise_load4<EXPL>(nz, 0);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 8) {
    const int dn = d0 + 8 < DAD_D ? d0 + 8 : d0;   // the last step reloads itself
    xn.load(store, xel + dn);
    nn = noise_load4<EXPL>(nz, dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D + dn);
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 x = xc.get();
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], wc[ht][e], acc0[ht], 0, 0, 0);
        acc1[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(nc[e], wc[ht][e], acc1[ht], 0, 0, 0);
      }
    xc = xn;
    nc = nn;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// eval_slab_f16 with the noise as a second fp16 A operand (rounded to fp16 like the rows)
template <int DT, bool EXPL>
__device__ __forceinline__ void eval_slab_noise_f16(const void* store, size_t xel, const NoiseSrc& nz,
                                                    const uint16_t* W, f32x16 (&acc0)[DAD_HT],
                                                    f32x16 (&acc1)[DAD_HT]) {
  Raw8<DT> xc, xn;
  u32x4 nc, nn;
  u32x4 wc[DAD_HT], wn[DAD_HT];
  xc.load(store, xel);
  nc = noise_frag8<EXPL>(nz, 0);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 16) {
    const int dn = d0 + 16 < DAD_D ? d0 + 16 : d0;
    xn.load(store, xel + dn);
    nn = noise_frag8<EXPL>(nz, dn);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D + dn);
    __builtin_amdgcn_sched_barrier(0);
    const f16x8 x = __builtin_bit_cast(f16x8, xc.frag());
    const f16x8 z = __builtin_bit_cast(f16x8, nc);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) {
      const f16x8 w = __builtin_bit_cast(f16x8, wc[ht]);
      acc0[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, w, acc0[ht], 0, 0, 0);
      acc1[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(z, w, acc1[ht], 0, 0, 0);
    }
    xc = xn;
    nc = nn;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// ---- an explicit perturbation added to the rows before the GEMM (input_grad.hip) ---------------------------
// The 8 channels of a Raw8 chunk widened to f32 (the values Raw4::get gives for the same channels)
template <int DT>
__device__ __forceinline__ void raw8_widen(const Raw8<DT>& r, f32x4& a, f32x4& b) {
  if constexpr (DT == DAD_STORE_F32) {
    a = r.a; b = r.b;
  } else if constexpr (DT == DAD_STORE_F16) {
    a[0] = Raw4<DAD_STORE_F16>::h(r.v[0] & 0xffffu); a[1] = Raw4<DAD_STORE_F16>::h(r.v[0] >> 16);
    a[2] = Raw4<DAD_STORE_F16>::h(r.v[1] & 0xffffu); a[3] = Raw4<DAD_STORE_F16>::h(r.v[1] >> 16);
    b[0] = Raw4<DAD_STORE_F16>::h(r.v[2] & 0xffffu); b[1] = Raw4<DAD_STORE_F16>::h(r.v[2] >> 16);
    b[2] = Raw4<DAD_STORE_F16>::h(r.v[3] & 0xffffu); b[3] = Raw4<DAD_STORE_F16>::h(r.v[3] >> 16);
  } else {
    a[0] = __uint_as_float(r.v[0] << 16); a[1] = __uint_as_float(r.v[0] & 0xffff0000u);
    a[2] = __uint_as_float(r.v[1] << 16); a[3] = __uint_as_float(r.v[1] & 0xffff0000u);
    b[0] = __uint_as_float(r.v[2] << 16); b[1] = __uint_as_float(r.v[2] & 0xffff0000u);
    b[2] = __uint_as_float(r.v[3] << 16); b[3] = __uint_as_float(r.v[3] & 0xffff0000u);
  }
}

// eval_slab_f32 (one network) on the rows x + delta: delta is an explicit f32 array in the slab-aligned layout of
// dad_eval_noise and del the element of the lane's first channel.  The sum is formed in f32 ahead of the MFMA, in
// eval_slab_f32's k order.
template <int DT>
__device__ __forceinline__ void eval_slab_delta_f32(const void* store, size_t xel, const float* delta, size_t del,
                                                    const float* W, f32x16 (&acc)[DAD_HT]) {
  Raw4<DT> xc, xn;
  f32x4 dc, dn;
  f32x4 wc[DAD_HT], wn[DAD_HT];
  xc.load(store, xel);
  dc = *reinterpret_cast<const f32x4*>(delta + del);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 8) {
    const int dn_ = d0 + 8 < DAD_D ? d0 + 8 : d0;   // the last step reloads itself
    xn.load(store, xel + dn_);
    dn = *reinterpret_cast<const f32x4*>(delta + del + dn_);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const f32x4*>(W + (size_t)ht * 32 * DAD_D + dn_);
    __builtin_amdgcn_sched_barrier(0);
    const f32x4 x = xc.get() + dc;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], wc[ht][e], acc[ht], 0, 0, 0);
    xc = xn;
    dc = dn;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// eval_slab_f16 (one network) on the rows x + delta: the f32 sum of the widened row and delta is rounded once to
// fp16
template <int DT>
__device__ __forceinline__ void eval_slab_delta_f16(const void* store, size_t xel, const float* delta, size_t del,
                                                    const uint16_t* W, f32x16 (&acc)[DAD_HT]) {
  Raw8<DT> xc, xn;
  f32x4 dc[2], dn[2];
  u32x4 wc[DAD_HT], wn[DAD_HT];
  xc.load(store, xel);
  dc[0] = *reinterpret_cast<const f32x4*>(delta + del);
  dc[1] = *reinterpret_cast<const f32x4*>(delta + del + 4);
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D);
  for (int d0 = 0; d0 < DAD_D; d0 += 16) {
    const int dn_ = d0 + 16 < DAD_D ? d0 + 16 : d0;
    xn.load(store, xel + dn_);
    dn[0] = *reinterpret_cast<const f32x4*>(delta + del + dn_);
    dn[1] = *reinterpret_cast<const f32x4*>(delta + del + dn_ + 4);
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wn[ht] = *reinterpret_cast<const u32x4*>(W + (size_t)ht * 32 * DAD_D + dn_);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 a, b;
    raw8_widen<DT>(xc, a, b);
    a += dc[0];
    b += dc[1];
    const f16x8 x = __builtin_bit_cast(f16x8, u32x4{dad_pack2<true>(a[0], a[1]), dad_pack2<true>(a[2], a[3]),
                                                    dad_pack2<true>(b[0], b[1]), dad_pack2<true>(b[2], b[3])});
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
      acc[ht] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, wc[ht]), acc[ht], 0, 0, 0);
    xc = xn;
    dc[0] = dn[0];
    dc[1] = dn[1];
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) wc[ht] = wn[ht];
  }
}

// eval_epilogue on acc0 + sigma[k] acc1 for every level k -> part[k][256] (one fma; sigma = 0 with a finite acc1
// leaves eval_epilogue's bits).  MAXK >= levels.  The level loop is unrolled into straight-line code behind
// wave-uniform branches, one h tile at a time, so the accumulators are copied to VALU registers 32 at a time next
// to their use and not all 256 ahead of a loop.
template <int MAXK>
__device__ __forceinline__ void eval_epilogue_noise(const f32x16* acc0, const f32x16* acc1, const float* sigma,
                                                    int levels, const float* bias, float* part, uint32_t vbits) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    const float bh = bias[ht * 32 + j];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      if (k >= levels) break;
      const float sg = sigma[k];
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool v = (vbits >> dad_acc_row(r, kh)) & 1u;
        const float pre = fmaf(sg, acc1[ht][r], acc0[ht][r]) + bh;
        s += (v && !(pre <= 0.0f)) ? pre : 0.0f;   // ReLU that keeps a NaN
      }
      s += __shfl_xor(s, 32, 64);
      if (kh == 0) part[(size_t)k * DAD_H + ht * 32 + j] = s;
    }
  }
}

}  // namespace

#endif  // DAD_EVAL_ROWS_H_
