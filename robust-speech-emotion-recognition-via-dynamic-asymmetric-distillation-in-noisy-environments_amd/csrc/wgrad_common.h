// Encoder weight gradient: dW1 = sum_rows G[row]^T x[row],  G = relu'(pre) * valid * dL/de_b / len_b
// (autograd of pre_net + ReLU + masked mean pool, I/model.py:28-36, for the clean branch
// (I/train.py:399) and the strong-augmented noisy branch (I/train.py:439)).
//
// K = rows (B*T per branch) is long and the output (256x768) small, so the reduction is
// split over `splits` row ranges; each workgroup writes one f32 partial slab, and
// dad_reduce sums them in a fixed order (deterministic, no float atomics).
// G is rebuilt on the fly from the ReLU' bit mask written by the forward and the
// per-(utterance, h) scale dL/de / len.  The strong branch's augmented input is
//   FP32: regenerated exactly (same counter-RNG function, or re-read explicit noise);
//   FP16/BF16: re-read from the 16-bit copy the forward stored (the exact MFMA operand it used).
// Both run after the losses as one direct split-K GEMM with the loss scale folded into G.
//
// Shared by the units of the family (wgrad_f32.hip, wgrad_direct.hip, wgrad_direct_rg.hip, reduce.hip):
// the fused dL/de, the slab list helpers and the extra block.
#pragma once
#include "dad_common.h"
#include "dad_kernels.h"

namespace {

// slab range [s0, s1) of a split of the dense list: a contiguous share of all slabs (past the list's end
// s0 > s1: the callers test s0 < s1; the ragged list's share: dad_wg_share)
__device__ __forceinline__ void wg_range(const DadWgradArgs& a, int split, int& s0, int& s1) {
  const int total = dad_wg_total(a.g, a.warmup);
  const int per = (total + a.splits - 1) / a.splits;
  s0 = split * per;
  s1 = min(total, s0 + per);
}

// slab s of the weight-gradient row list: clean slabs first, then strong (noisy) slabs
struct SlabIdx {
  int br, b, c, T;
  int erow;          // row of ge / vlen (clean b, or Bc + b)
  size_t row0;       // [b][T] row of frame 0
  size_t bits_slab;  // slab index in the ReLU' row-mask buffer (= s)
};
__device__ __forceinline__ SlabIdx wg_slab(const DadGeom& g, int s) {
  const int nsc = g.Bc * g.ncc;
  SlabIdx r;
  r.br = s >= nsc;
  const int rem = r.br ? s - nsc : s;
  const int nc = r.br ? g.ncn : g.ncc;
  r.b = rem / nc;
  r.c = rem - r.b * nc;
  r.T = r.br ? g.Tn : g.Tc;
  r.erow = r.br ? g.Bc + r.b : r.b;
  r.row0 = (size_t)r.b * r.T;
  r.bits_slab = (size_t)s;
  return r;
}

// Fused step: dL/de of utterance row u (clean u < Bc, strong Bc + b), hidden unit h: the
// classifier part keep(u,h) * sum_c W2[c][h] dL/dz[u][c] (nn.Linear + nn.Dropout backward,
// I/model.py:62-63) plus the ECDA part where ECDA wrote the row.
// ec = ge_ecda[u][h] as loaded by the caller (read whatever the flag: unflagged rows hold
// stale values and are selected away, so a caller can keep all its loads in flight)
// EX: explicit dropout masks (a.keep1 set), chosen by the caller outside its loops
// (gz = dL/dz[u], ef = eflag[u], ec as loaded by the caller)
template <bool EX>
__device__ __forceinline__ float fused_ge1_v(const DadReduceArgs& a, int Bc, int u, int h, const float (&w2)[4],
                                             const f32x4& gz, uint32_t ef, float ec, float* kv_out = nullptr) {
  const bool strong = u >= Bc;
  const int b = strong ? u - Bc : u;
  const float kv = keep_value_t<EX>(strong ? a.keep2 : a.keep1, strong ? a.key_drop2 : a.key_drop1, b, h, a.p_drop,
                                    a.drop_scale);
  if (kv_out) *kv_out = kv;
  const float z = ((w2[0] * gz[0] + w2[1] * gz[1]) + w2[2] * gz[2]) + w2[3] * gz[3];
  return z * kv + (ef ? ec : 0.0f);
}
template <bool EX>
__device__ __forceinline__ float fused_ge1_ec(const DadReduceArgs& a, int Bc, int u, int h, const float (&w2)[4],
                                              float ec, float* kv_out = nullptr) {
  return fused_ge1_v<EX>(a, Bc, u, h, w2, *reinterpret_cast<const f32x4*>(a.gzb + (size_t)u * DAD_C), a.eflag[u], ec,
                         kv_out);
}
template <bool EX>
__device__ __forceinline__ float fused_ge1(const DadReduceArgs& a, int Bc, int u, int h, const float (&w2)[4],
                                           float* kv_out = nullptr) {
  return fused_ge1_ec<EX>(a, Bc, u, h, w2, a.ge_ecda[(size_t)u * DAD_H + h], kv_out);
}

}  // namespace

// blocks NB + e, e < DAD_REDUCE_XBLK: hidden units 16e .. 16e+15 of
//   db1[h]    = sum_r dL/de[r][h] / max(1, len_r) * active_count[r][h]      (autograd of b1)
//   dW2[c][h] = sum_r dL/dz[r][c] * dropout(e_r)[h]   (fused step; the tail no longer does it)
// their squared-norm share, and (e = 0) the b2 norm share and the loss totals
// (I/train.py:462-466).  Thread = (hidden unit hl, row group rg): rows rg, rg+16, ...;
// the 16 row groups are combined in fixed order (deterministic).
static_assert(DAD_REDUCE_THREADS == 256 && DAD_H == 16 * DAD_REDUCE_XBLK, "extra blocks: 16 h x 16 row groups");

// run by 256 threads (tid = 0..255 of a workgroup or of half of one), combining in xs
template <bool EX>
__device__ double extra_block_t(const DadReduceArgs& a, int e, int tid, float (*xs)[16][6]) {
  const int hl = tid & 15, rg = tid >> 4;
  const int h = 16 * e + hl;
  const DadGeom& g = a.g;
  const int nb = g.Bc + (a.warmup ? 0 : g.Bn);
  const bool fused = a.gzb != nullptr;
  const bool ecda = a.ge_ecda != nullptr;
  float w2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (fused)
#pragma unroll
    for (int c = 0; c < 4; ++c) w2[c] = a.student[DAD_OFF_W2 + c * DAD_H + h];
  float db = 0.0f, gw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  // rows rg, rg + 16, ... in batches of 8 whose loads are all issued before any is used
  // (index clamped, contribution masked): one memory round trip per batch, not per row
  for (int r0 = rg; r0 < nb; r0 += 16 * 8) {
    float gv[8], kv[8], rl[8], ct[8], em[8];
    f32x4 gzv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = min(r0 + 16 * k, nb - 1);
      kv[k] = 1.0f;
      if (fused) {
        gv[k] = fused_ge1<EX>(a, g.Bc, r, h, w2, &kv[k]);
        const int erow = r >= g.Bc ? g.Bn + r : r;   // strong row b lives at Bc + Bn + b
        em[k] = a.emb[(size_t)erow * DAD_H + h];
        gzv[k] = *reinterpret_cast<const f32x4*>(a.gzb + (size_t)r * DAD_C);
      } else {
        gv[k] = a.ge[(size_t)r * DAD_H + h];
        if (ecda) gv[k] += a.ge_ecda[(size_t)r * DAD_H + h];
        em[k] = 0.0f;
        gzv[k] = f32x4{};
      }
      rl[k] = a.vlen[r];
      ct[k] = a.cnt_tot[(size_t)r * DAD_H + h];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (r0 + 16 * k >= nb) break;
      db += gv[k] / fmaxf(rl[k], 1.0f) * ct[k];
      if (fused) {
        // dW2[c][h] = sum_u dL/dz[u][c] * dropout(e_u)[h]  (student clean / strong embeddings)
        const float d = em[k] * kv[k];
#pragma unroll
        for (int c = 0; c < 4; ++c) gw[c] += gzv[k][c] * d;
      }
    }
  }
  xs[rg][hl][0] = db;
#pragma unroll
  for (int c = 0; c < 4; ++c) xs[rg][hl][1 + c] = gw[c];
  __syncthreads();
  double sq = 0.0;
  if (tid < 16 * 5) {
    const int k = tid >> 4, hh = tid & 15;   // k: 0 = db1, 1..4 = dW2 row c = k-1
    float v = xs[0][hh][k];
    for (int q = 1; q < 16; ++q) v += xs[q][hh][k];
    if (k == 0) {
      a.grad[DAD_OFF_B1 + 16 * e + hh] = v;
      sq = (double)v * v;
    } else if (a.tailf) {
      if (fused) a.grad[DAD_OFF_W2 + (k - 1) * DAD_H + 16 * e + hh] = v;
      else v = a.grad[DAD_OFF_W2 + (k - 1) * DAD_H + 16 * e + hh];
      sq = (double)v * v;
    }
  }
  if (e == 0 && a.tailf && tid >= 96 && tid < 100) {
    const float gb = a.grad[DAD_OFF_B2 + tid - 96];
    sq += (double)gb * gb;
  }
  if (e == 0 && a.tailf && tid == 128) {
    const float* tf = a.tailf;
    const float ecda_l = ((tf[DAD_T_ECDA_TERM] + tf[DAD_T_ECDA_TERM + 1]) + tf[DAD_T_ECDA_TERM + 2]) +
                         tf[DAD_T_ECDA_TERM + 3];
    const float ce = tf[DAD_T_CE], kl = tf[DAD_T_KL];
    float* ex = a.grad + DAD_NPARAM;
    // a pooling timeout in the tail launch (DAD_POOL_ABORT): NaN total, so dad_optim (on every DP
    // rank, after the all-reduce) skips this step's update
    const bool abort = a.pool_abort != nullptr && __hip_atomic_load(a.pool_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    // (the supervised-contrastive term: written behind the tail launch by dad_scl_final; without it 0 * 0)
    ex[12] = abort ? __builtin_nanf("") : ce + a.w_kl * kl + a.w_ecda * ecda_l + a.w_scl * tf[DAD_T_SCL];
    ex[13] = ce;
    ex[14] = kl;
    ex[15] = ecda_l;
  }
  return sq;
}
static __device__ double extra_block(const DadReduceArgs& a, int e, int tid, float (*xs)[16][6]) {
  return a.keep1 ? extra_block_t<true>(a, e, tid, xs) : extra_block_t<false>(a, e, tid, xs);
}
