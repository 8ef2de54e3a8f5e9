// dad_wgrad_f32: the exact-f32 weight gradient of the parity mode (the family: wgrad_common.h)
#include "wgrad_common.h"
#include "dad_prep.h"

namespace {

__device__ __forceinline__ float wg_featkeep(const DadWgradArgs& a, int d) {
  return dad_feat_keep(a.u, a.key_feat, d, a.feat_p);
}

}  // namespace

// ------------------------------------------------------------------- FP32 (parity mode)
// grid = 6 column blocks x splits; wave = 32 columns x 256 rows of dW1.
// v_mfma_f32_32x32x2_f32: A[i=h][k] = G[row k][h], B[k][j=d] = x[row k][d] (k = 2 rows).
//
// An f32 MFMA holds the SIMD's vector issue for its whole 64 cycles (PMC: zero VALU/MFMA
// co-execution cycles), so every VALU instruction of the loop adds its 4+ cycles to the
// MFMA time: the loop is built to issue as few as possible per MFMA.
//   * G (256 h x 32 rows of the slab, = ReLU' bit ? dL/de_u[h] / len_u : 0) is built ONCE per
//     workgroup into LDS (thread = h, double-buffered, one barrier per slab) and read as MFMA
//     A operands with ds_read_b128 (4 row pairs per read), instead of every wave rebuilding
//     all of it per MFMA (select + scale: 2-3 VALU per MFMA, and the fused dL/de per h).
//   * x (rows 2j + kh at column d) is loaded one slab ahead through a buffer descriptor of the
//     slab's valid rows (rows past the utterance read 0; one add per load for the address).
// The strong branch's augmentation is regenerated per element (counter RNG or explicit noise).
constexpr int F32_GP = 36;   // G tile pitch per h: [kh][16 pairs] + 4 floats (conflict-free b128 reads)

// the scale of G: dL/de / len from a dL/de buffer (modular encoder backward), or rebuilt from
// the tail's dL/dz and the ECDA rows (fused step, fused_ge1)
enum { F32_GE = 1, F32_FUSED = 2 };

struct F32X {
  float x[16], n[16];
};

// this lane's x (and explicit noise) of slab s: rows 2j + kh, column d
template <bool EXPLICIT, bool STORE>
__device__ __forceinline__ void f32_xload(const DadWgradArgs& a, int s, int d, int kh, F32X& r) {
  const SlabIdx q = wg_slab(a.g, s);
  const int nval = min(DAD_SLAB, q.T - q.c * DAD_SLAB);   // rows of the slab inside the utterance
  if constexpr (!STORE) {
    const float* X = (q.br ? a.xn : a.xc) + (q.row0 + (size_t)q.c * DAD_SLAB) * DAD_D;
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X), 0, nval * DAD_D * 4, 0x00020000);
    // The row offset goes in voffset, not soffset: the range check compares voffset (+ the
    // instruction offset) with num_records, so rows past the utterance read 0 and nothing is
    // read past the slab.  (The builtin returns the raw bits: __uint_as_float, not a value
    // conversion.)
    const int vo = (kh * DAD_D + d) * 4;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      r.x[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vo + j * 2 * DAD_D * 4, 0, 0));
    if constexpr (EXPLICIT) {
      const float* N = a.ns + (q.row0 + (size_t)q.c * DAD_SLAB) * DAD_D;
      const auto rn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(N), 0, nval * DAD_D * 4, 0x00020000);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        r.n[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rn, vo + j * 2 * DAD_D * 4, 0, 0));
    }
  } else {
    const float* X = q.br ? a.xn : a.xc;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int t = min(q.c * DAD_SLAB + 2 * j + kh, q.T - 1);
      r.x[j] = X[dad_src_row(a.src, q.br, q.b, q.T, t) * DAD_D + d];
      if constexpr (EXPLICIT) r.n[j] = a.ns[(q.row0 + t) * DAD_D + d];
    }
  }
}

// G inputs of thread h for slab s: the ReLU' row mask and the ECDA row / dL/de value
struct F32GIn {
  uint32_t mw;
  float ec;
};
template <int MODE>
__device__ __forceinline__ void f32_gload(const DadWgradArgs& a, const DadReduceArgs& ra, int s, int h, F32GIn& r) {
  const SlabIdx q = wg_slab(a.g, s);
  r.mw = a.bits[q.bits_slab * DAD_H + h];
  r.ec = 0.0f;
  if constexpr (MODE == F32_GE) r.ec = a.ge[(size_t)q.erow * DAD_H + h];
  if constexpr (MODE == F32_FUSED) r.ec = ra.ge_ecda[(size_t)q.erow * DAD_H + h];
}

// G^T of slab s into LDS: thread h writes G[h][kh][j] = bit (2j + kh) of its mask ? scale : 0
template <int MODE, bool KEEPX>
__device__ __forceinline__ void f32_gbuild(const DadWgradArgs& a, const DadReduceArgs& ra, int s, int h,
                                           const float (&w2h)[4], const F32GIn& gi, float* G) {
  const SlabIdx q = wg_slab(a.g, s);
  float scale = 0.0f;
  if constexpr (MODE == F32_GE) scale = gi.ec / fmaxf(a.vlen[q.erow], 1.0f);
  if constexpr (MODE == F32_FUSED) {
    // dL/de_u[h] / max(1, len_u), as dad_wgrad_direct builds it (16-bit there, f32 here)
    const int u = q.erow;
    const f32x4 gz = *reinterpret_cast<const f32x4*>(ra.gzb + (size_t)u * DAD_C);
    scale = fused_ge1_v<KEEPX>(ra, a.g.Bc, u, h, w2h, gz, ra.eflag[u], gi.ec) / fmaxf(ra.vlen[u], 1.0f);
  }
  const uint32_t sb = __float_as_uint(scale);
#pragma unroll
  for (int kh = 0; kh < 2; ++kh)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = __uint_as_float((uint32_t)__builtin_amdgcn_sbfe((int)gi.mw, 2 * (4 * q4 + e) + kh, 1) & sb);
      *reinterpret_cast<f32x4*>(G + h * F32_GP + kh * 16 + 4 * q4) = v;
    }
}

// one slab's 128 MFMAs of this wave: A from the LDS G tile, B = x (strong: augmented here)
template <bool EXPLICIT, bool STRONG>
__device__ __forceinline__ void f32_mma(const DadWgradArgs& a, const SlabIdx& q, int d, int kh, float fkeep, int st,
                                        const float* G, const F32X& r, f32x16 (&acc)[DAD_HT]) {
  const int lane = threadIdx.x & 63;
  const float* gl = G + (lane & 31) * F32_GP + kh * 16;
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    f32x4 gv[DAD_HT];
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) gv[ht] = *reinterpret_cast<const f32x4*>(gl + ht * 32 * F32_GP + 4 * q4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * q4 + e;
      float x = r.x[j];
      if constexpr (STRONG) {
        const int t = q.c * DAD_SLAB + 2 * j + kh;
        const bool tin = t < q.T;
        const size_t grow = q.row0 + (tin ? t : 0);
        const float n = EXPLICIT ? r.n[j] : dad_normal1(a.key_strong, (uint32_t)(grow * DAD_D + d));
        const float sn = n * a.strong_std;
        x = (x + sn) * fkeep;
        x = (t >= st && t < st + a.mask_len) ? 0.0f : x;   // (st + mask_len <= st when mask_len = 0)
        x = tin ? x : 0.0f;
      }
#pragma unroll
      for (int ht = 0; ht < DAD_HT; ++ht) acc[ht] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[ht][e], x, acc[ht], 0, 0, 0);
    }
  }
}

template <bool EXPLICIT, int MODE, bool STORE, bool KEEPX>
__device__ __forceinline__ void wgrad_f32_body(const DadWgradArgs& a, const DadReduceArgs& ra, float* Gs) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = lane & 31, kh = lane >> 5;
  const int h = tid;   // (256 threads = the 256 hidden units, for the G tile)
  float w2h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (MODE == F32_FUSED)
#pragma unroll
    for (int c = 0; c < 4; ++c) w2h[c] = ra.student[DAD_OFF_W2 + c * DAD_H + h];
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int dblk = tile % 6, split = tile / 6;
    const int d = (dblk * 4 + wv) * 32 + i;
    int s0, s1;
    wg_range(a, split, s0, s1);
    f32x16 acc[DAD_HT];
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht) acc[ht] = f32x16{};
    const float fkeep = wg_featkeep(a, d);   // (the strong branch's feature mask; clean rows ignore it)
    if (s0 < s1) {
      F32GIn gi, gn;
      F32X cur, nxt;
      f32_gload<MODE>(a, ra, s0, h, gi);
      f32_xload<EXPLICIT, STORE>(a, s0, d, kh, cur);
      f32_gload<MODE>(a, ra, min(s0 + 1, s1 - 1), h, gn);
      f32_gbuild<MODE, KEEPX>(a, ra, s0, h, w2h, gi, Gs);
      f32_xload<EXPLICIT, STORE>(a, min(s0 + 1, s1 - 1), d, kh, nxt);
      __syncthreads();
      for (int s = s0; s < s1; ++s) {
        const int buf = (s - s0) & 1;
        const SlabIdx q = wg_slab(a.g, s);
        const float* G = Gs + buf * (DAD_H * F32_GP);
        if (q.br) {
          const int st = a.mask_len > 0 ? (EXPLICIT ? (int)a.start[q.b] : dad_tstart_at(a.key_tstart, q.b, a.start_hi)) : 0;
          f32_mma<EXPLICIT, true>(a, q, d, kh, fkeep, st, G, cur, acc);
        } else {
          f32_mma<EXPLICIT, false>(a, q, d, kh, fkeep, 0, G, cur, acc);
        }
        // the next slab's G (its inputs loaded a slab ago), then the loads of slab s + 2
        if (s + 1 < s1) f32_gbuild<MODE, KEEPX>(a, ra, s + 1, h, w2h, gn, Gs + (buf ^ 1) * (DAD_H * F32_GP));
        cur = nxt;
        f32_gload<MODE>(a, ra, min(s + 2, s1 - 1), h, gn);
        f32_xload<EXPLICIT, STORE>(a, min(s + 2, s1 - 1), d, kh, nxt);
        __syncthreads();
      }
    }
    float* out = a.wpart + (size_t)split * DAD_H * DAD_D;
#pragma unroll
    for (int ht = 0; ht < DAD_HT; ++ht)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(size_t)(ht * 32 + dad_acc_row(r, kh)) * DAD_D + d] = acc[ht][r];
  }
}

// KEEPX: explicit classifier-dropout masks (fused mode only)
template <bool EXPLICIT, int MODE, bool KEEPX>
__device__ __forceinline__ void wgrad_f32_store(const DadWgradArgs& a, const DadReduceArgs& ra, float* Gs) {
  if (a.src.rowc != nullptr) wgrad_f32_body<EXPLICIT, MODE, true, KEEPX>(a, ra, Gs);
  else wgrad_f32_body<EXPLICIT, MODE, false, KEEPX>(a, ra, Gs);
}
template <bool EXPLICIT>
__device__ __forceinline__ void wgrad_f32_mode(const DadWgradArgs& a, const DadReduceArgs& ra, float* Gs) {
  if (ra.gzb == nullptr) wgrad_f32_store<EXPLICIT, F32_GE, false>(a, ra, Gs);
  else if (ra.keep1) wgrad_f32_store<EXPLICIT, F32_FUSED, true>(a, ra, Gs);
  else wgrad_f32_store<EXPLICIT, F32_FUSED, false>(a, ra, Gs);
}

__global__ __launch_bounds__(DAD_WGRAD_THREADS) void dad_wgrad_f32(DadWgradArgs a, DadReduceArgs ra) {
  DAD_GUARD_BLOCK(DAD_WGRAD_THREADS);
  static_assert(DAD_WGRAD_THREADS == DAD_H, "dad_wgrad_f32: thread = hidden unit for the G tile");
  __shared__ __attribute__((aligned(16))) float Gs[2 * DAD_H * F32_GP];
  if (a.ns) wgrad_f32_mode<true>(a, ra, Gs);
  else wgrad_f32_mode<false>(a, ra, Gs);
}
