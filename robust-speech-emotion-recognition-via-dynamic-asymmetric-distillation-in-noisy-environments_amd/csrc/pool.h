// Pooling finalisation + classifier forward of one (utterance, branch), as device code shared by
// its two launches (header only):
//
//   pool_item<SC1>            e = sum(slab partials)/max(1,len)            I/model.py:35-36
//                             logits = W2 (dropout(e)) + b2                I/model.py:54-64
//                             one wave; dad_pool (tail_general.hip) runs it per workgroup with
//                             plain stores, dad_tail_ecda_w (tail_w.hip) on its spare
//                             workgroups' waves with write-through stores
//   pool_publish / pool_wait  the counter hand-off from those waves to the tail and class
//                             blocks of the same dad_tail_ecda_w launch
#pragma once
#include "dad_common.h"
#include "dad_kernels.h"

// One wave per (utterance, branch): blocks [0, Bc) clean, [Bc, Bc+Bn) teacher (weak),
// [Bc+Bn, Bc+2Bn) student (strong).  Lane l owns hidden units 4l..4l+3, so a slab partial is
// one 16-B load per lane, every load of the block (pad bytes, all slab partials in batches of
// POOL_BATCH, active counts, W2 columns) is issued before the first sum, and the length and
// the four logit dot products are wave reductions: no LDS, no barrier (the 256-thread form
// issued 48 dword loads per thread and joined its 4 waves through LDS twice).  Embeddings sum
// the slab partials in slab order (I/model.py:35-36 masked mean pooling); logits
// W2 . dropout(e) + b2 (I/model.py:54-64; the teacher classifier's dropout is off).
//
// The same item runs in dad_tail_ecda_w's spare workgroups (SC1 = true: the tail and class
// blocks of that launch read the results after a counter hand-off, so every store is
// write-through, MI355X_MICROARCH.md "Valid forms").
static_assert(DAD_POOL_THREADS == 64 && DAD_H == 4 * 64, "dad_pool: one wave, 4 hidden units per lane");

template <bool SC1>
__device__ __forceinline__ void pool_st4(float* p, const f32x4& v) {
  if constexpr (SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  else *reinterpret_cast<f32x4*>(p) = v;
}
template <bool SC1, class T>
__device__ __forceinline__ void pool_st1(T* p, T v) {
  if constexpr (SC1) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// pool item blk (one wave, lane = 0..63): what one dad_pool workgroup does
// RG (the ragged step's kernels): the encoder wrote the partials of the utterance's live slabs only
// (c < ceil(len_b / 32), len_b from a.lenc / a.lenn), so only those are summed, in the same slab order;
// the dead slabs' partials of the dense step are exact zeros, so the sums are the same bits.
template <bool SC1, bool RG = false>
__device__ __forceinline__ void pool_item(const DadPoolArgs& a, const int blk, const int lane) {
  const DadGeom& g = a.g;
  const int kind = blk < g.Bc ? 0 : (blk < g.Bc + g.Bn ? 1 : 2);   // clean, teacher (weak), student (strong)
  const int b = kind == 0 ? blk : (kind == 1 ? blk - g.Bc : blk - g.Bc - g.Bn);
  const bool noisy = kind != 0, teacher = kind == 1;
  const int T = noisy ? g.Tn : g.Tc;
  const uint8_t* pad = (noisy ? a.mn : a.mc) + (size_t)b * T;
  const size_t nsc = (size_t)g.Bc * g.ncc, nsn = (size_t)g.Bn * g.ncn;
  int nc = noisy ? g.ncn : g.ncc;
  int clast = nc - 1;      // slab index the batched loads are clamped to
  if constexpr (RG) {
    nc = dad_live_slabs((noisy ? a.lenn : a.lenc)[b], nc);
    clast = max(nc - 1, 0);   // (no live slab: slab 0's address, loaded and selected away)
  }
  const size_t slab0 = kind == 0 ? (size_t)b * g.ncc : (kind == 1 ? nsc + (size_t)b * g.ncn : nsc + nsn + (size_t)b * g.ncn);
  const size_t cslab0 = noisy ? nsc + (size_t)b * g.ncn : (size_t)b * g.ncc;   // active counts (clean / strong)
  const int erow = kind == 0 ? b : (kind == 1 ? g.Bc + b : g.Bc + g.Bn + b);
  const int h0 = 4 * lane;
  // First batch, every load issued before any sum: the pad bytes of frames lane + 64k (k <
  // POOL_PADB: T <= 512), the slab partials and active counts of slabs 0 .. POOL_BATCH-1 (index
  // clamped, contribution masked; summed in slab order).  (A pad loop with the sum inside waited
  // on each byte before the next load: one memory round trip per 64 frames, ahead of the slab
  // loads.)  The teacher also loads the strong counts it does not use: no load under a branch.
  constexpr int POOL_PADB = 8, POOL_BATCH = 16;
  uint8_t pv[POOL_PADB];
#pragma unroll
  for (int k = 0; k < POOL_PADB; ++k) pv[k] = pad[min(lane + 64 * k, T - 1)];
  f32x4 ps[POOL_BATCH], pc[POOL_BATCH];
#pragma unroll
  for (int k = 0; k < POOL_BATCH; ++k) {
    const int c = min(k, clast);
    ps[k] = *reinterpret_cast<const f32x4*>(a.part_sum + (slab0 + c) * DAD_H + h0);
    pc[k] = *reinterpret_cast<const f32x4*>(a.part_cnt + (cslab0 + c) * DAD_H + h0);
  }
  // valid length (I/model.py:35: (1-mask).sum(dim=1)); frames past the first batch in a loop
  float len = 0.0f;
#pragma unroll
  for (int k = 0; k < POOL_PADB; ++k) len += ((lane + 64 * k < T) & (pv[k] == 0)) ? 1.0f : 0.0f;
  for (int t = lane + 64 * POOL_PADB; t < T; t += 64) len += pad[t] == 0 ? 1.0f : 0.0f;
  f32x4 ssum = f32x4{}, cnt = f32x4{};
#pragma unroll
  for (int k = 0; k < POOL_BATCH; ++k) {   // (+0 past the utterance's slabs: the sums are unchanged)
    const bool in = k < nc;
    ssum += in ? ps[k] : f32x4{};
    cnt += in ? pc[k] : f32x4{};
  }
  for (int c0 = POOL_BATCH; c0 < nc; c0 += POOL_BATCH) {   // utterances past 512 frames
#pragma unroll
    for (int k = 0; k < POOL_BATCH; ++k) {
      const int c = min(c0 + k, clast);
      ps[k] = *reinterpret_cast<const f32x4*>(a.part_sum + (slab0 + c) * DAD_H + h0);
      pc[k] = *reinterpret_cast<const f32x4*>(a.part_cnt + (cslab0 + c) * DAD_H + h0);
    }
#pragma unroll
    for (int k = 0; k < POOL_BATCH; ++k) {
      const bool in = c0 + k < nc;
      ssum += in ? ps[k] : f32x4{};
      cnt += in ? pc[k] : f32x4{};
    }
  }
  const float* par = teacher ? a.teacher : a.student;
  f32x4 w2[DAD_C];
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) w2[c] = *reinterpret_cast<const f32x4*>(par + DAD_OFF_W2 + c * DAD_H + h0);
  const float bias = par[DAD_OFF_B2 + (lane & (DAD_C - 1))];
  f32x4 kv;
#pragma unroll
  for (int e = 0; e < 4; ++e)   // teacher classifier: dropout p = 0 (I/model.py:121); students: masks #1 / #2
    kv[e] = teacher ? 1.0f
                    : (kind == 0 ? keep_value(a.keep1, a.key_drop1, b, h0 + e, a.p_drop, a.drop_scale)
                                 : keep_value(a.keep2, a.key_drop2, b, h0 + e, a.p_drop, a.drop_scale));
  len = dad_wave_sum(len);
  f32x4 e;
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = ssum[k] / fmaxf(len, 1.0f);
  pool_st4<SC1>(a.emb + (size_t)erow * DAD_H + h0, e);
  const f32x4 d = teacher ? e : e * kv;
  float zp[DAD_C];
#pragma unroll
  for (int c = 0; c < DAD_C; ++c)
    zp[c] = dad_wave_sum(((w2[c][0] * d[0] + w2[c][1] * d[1]) + w2[c][2] * d[2]) + w2[c][3] * d[3]);
  if (lane < DAD_C)
    pool_st1<SC1>(a.logits + (size_t)erow * DAD_C + lane, (lane == 0 ? zp[0] : (lane == 1 ? zp[1] : (lane == 2 ? zp[2] : zp[3]))) + bias);
  // range check: a non-finite embedding or logit sets the sticky flag.  In FP16 steps an encoder
  // operand beyond +-65504 converts to inf, which turns every pre-activation of its row into
  // +-inf or NaN: the +inf units survive the ReLU into the pooled sum.
  const bool fin = __builtin_isfinite(e[0]) & __builtin_isfinite(e[1]) & __builtin_isfinite(e[2]) &
                   __builtin_isfinite(e[3]) & __builtin_isfinite(((zp[0] + zp[1]) + zp[2]) + zp[3]);
  if (__ballot(!fin) != 0 && lane == 0 && a.range_flag)
    __hip_atomic_fetch_or(a.range_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!teacher) {
    // active-row count per (utterance, h) of the branch that gets a gradient (clean / strong);
    // the length, and the ECDA row flag (clean b / noisy Bc + b) starts at zero: the ECDA
    // workgroups write only what they own
    const int urow = noisy ? g.Bc + b : b;
    pool_st4<SC1>(a.cnt_tot + (size_t)urow * DAD_H + h0, cnt);
    if (lane == 0) {
      pool_st1<SC1>(a.vlen + urow, len);
      pool_st1<SC1>(a.eflag + urow, 0u);
    }
  }
  if (blk == 0 && lane < 2 * DAD_C) pool_st1<SC1>(a.tail_terms + lane, 0.0f);   // per-class ECDA terms and gates
}

// Fused pooling hand-off (dad_tail_ecda_w): each pooling wave stores its item write-through (sc1),
// drains (s_waitcnt vmcnt(0)) and adds 1 to the counter; a tail / class block polls the counter
// (one lane, sc1 loads), then ONE agent-scope acquire, a drain and a barrier before any of its
// waves loads (MI355X_MICROARCH.md "Valid forms": producer sc1 stores, consumer poll + acquire).
// The poll is bounded (~0.2 s); on timeout it sets bit 1 of the range flag and the step's abort
// word and goes on (no hung device): the block then computes on partly pooled rows, but the
// weight gradient's loss-total block turns the total loss into NaN and dad_optim leaves the
// parameters, moments, teacher and DACP state of that step untouched.
// The counter is sharded per XCD (DAD_POOL_SHARDS words, each on a 128-B line of its own: the
// arrivals of one XCD serialise on one line only) and a poll sums the shards.
__device__ __forceinline__ void pool_publish(uint32_t* ready, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) {
    const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & (DAD_POOL_SHARDS - 1);   // HW_REG_XCC_ID
    __hip_atomic_fetch_add(ready + 32 * xcc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ __forceinline__ void pool_wait(uint32_t* ready, uint32_t n, uint32_t* range_flag) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    uint32_t spins = 0;
    for (;;) {
      const uint32_t v = lane < DAD_POOL_SHARDS ? __hip_atomic_load(ready + 32 * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      if ((uint32_t)dad_wave_sum((float)v) >= n) break;   // (exact: at most a few hundred arrivals)
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1u << 23)) {
        if (lane == 0) {   // bit 1 of the sticky flag, and this step's abort word: no update (dad_optim)
          if (range_flag) __hip_atomic_fetch_or(range_flag, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(ready + DAD_POOL_ABORT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        break;
      }
    }
    if (lane == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}
