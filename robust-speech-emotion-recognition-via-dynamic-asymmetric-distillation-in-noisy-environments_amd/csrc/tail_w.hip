// The wave-centric tail launch dad_tail_ecda_w: the tail and ECDA of a step with at most 64
// utterances per side and class-aware MMD (the benchmark's geometry; tail_general.hip otherwise).
// One launch, grid 1 + C + spare:
//
//   block 0       tail_block_w   CE, teacher certainty, DACP mask, masked KL, dL/dz
//                                                          I/train.py:397-471, I/utils.py:400-507
//   blocks 1..C   ecda_block_w   ECDALoss forward + backward of class blockIdx.x - 1, Gram matrix
//                                and member gradients on the fp32 matrix cores  I/utils.py:510-652
//   blocks > C    the step's pooling (pool.h), handed to the blocks above through a counter, then
//                 the NEXT step's row preparation (dad_prep.h)
//
// The per-row arithmetic (CE row, KL row, class threshold) is tail_common.h's, shared with the
// general path; here a row is a lane and sums are wave reductions.  The phase stamps of the
// 'stamps' build (dad_probe.h) exist for this launch only; their buffers live in this unit.
#include "dad_prep.h"
#include "dad_probe.h"
#include "pool.h"
#include "tail_common.h"

// ECDA per-class phase wall clocks (100 MHz) of the stamps build (dad_probe.h): ECDA_SLOTS slots
// per class, then the tail block's phases
#define ECDA_SLOTS 32
DAD_PROBE_BUFFER(ecda_stamps, DAD_C * ECDA_SLOTS + 16)
// dad_tail_ecda_w's preparation waves (spare block xb < 256, wave w): [start, end] wall clocks
DAD_PROBE_BUFFER(prep_stamps, 256 * 8 * 2)
// class block blockIdx.x - 1
#define ECDA_STAMP(k) \
  if (threadIdx.x == 0) DAD_PROBE_SET(ecda_stamps, (blockIdx.x - 1) * ECDA_SLOTS + (k), DAD_PROBE_WALL())
// shader-clock stamp of wave 0 (cycle-level sub-phases of the stamps build), pinned in place
#define ECDA_CYC(k)                                                                          \
  do {                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    if (threadIdx.x == 0) DAD_PROBE_SET(ecda_stamps, (blockIdx.x - 1) * ECDA_SLOTS + (k), DAD_PROBE_CLK()); \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  } while (0)
#define ECDA_STAMP_SIZES(c, n, ns) \
  do { DAD_PROBE_SET(ecda_stamps, (c) * ECDA_SLOTS + 10, (n)); DAD_PROBE_SET(ecda_stamps, (c) * ECDA_SLOTS + 11, (ns)); } while (0)
#define TAIL_STAMP(k) \
  if (threadIdx.x == 0) DAD_PROBE_SET(ecda_stamps, DAD_C * ECDA_SLOTS + (k), DAD_PROBE_WALL())
// shader-clock cycles at the tail block's start / end (slots 12 / 13): with the wall-clock
// stamps 0 / 1 they give the clock the block ran at
#define TAIL_CYCLES(k) \
  if (threadIdx.x == 0) DAD_PROBE_SET(ecda_stamps, DAD_C * ECDA_SLOTS + (k), DAD_PROBE_CLK())

// stamp from wave 1's first lane (the tail block's DACP / KL wave)
#define TAIL_STAMP_W1(k) \
  if (threadIdx.x == 64 && blockIdx.x == 0) DAD_PROBE_SET(ecda_stamps, DAD_C * ECDA_SLOTS + (k), DAD_PROBE_WALL())

// =====================================================================================
// Same outputs as dad_tail_ecda (tail_general.hip), far fewer barrier-separated phases:
//  * DACP (I/utils.py:449-507) by the 8 waves of a block alike: lane i = noisy row i; each wave
//    counts an eighth of every row's rank by a readlane sweep, one barrier combines them, then
//    every wave sorts into its own table, lanes 0..3 take their class's threshold and readlane
//    broadcasts it (dacp_block8; the threshold is dacp_class_threshold, the general path's too,
//    so the masks are bit-identical).  Every wave of an ECDA block thus holds the mask itself.
//  * the tail block: CE in wave 0 (lane = clean row), teacher certainty + DACP + KL in wave 1
//    (lane = noisy row), wave reductions by DPP, one barrier to combine.
//  * an ECDA class block stages its CANDIDATE rows (clean label c, masked-in noisy rows of
//    pseudo-label c) from the registers they were prefetched into; the pairwise distances
//    come from a Gram matrix on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, K split over
//    the 8 waves), D_ij = |z_i|^2 + |z_j|^2 - 2 z_i.z_j; the member gradients
//    2 sum_j C_ij (z_i - z_j) = 2 (rowsum(C)_i z_i - (C Z)_i) are a second MFMA GEMM.
//    Four workgroup barriers in all.  A class with more than 64 candidates (up to 128) takes
//    ecda_class_w<true>: the same passes with its rows read from the embedding buffer, not LDS.
// =====================================================================================
#define TW_MAXB 64
// Pitches (floats) of the staged rows and the coefficient matrix: multiples of 4 (16-B rows) with
// pitch/4 odd, so the MFMA operand reads -- one ds_read_b128 of 4 consecutive k per lane, the
// 32 lanes of a half on 32 different rows -- fall on 16 different 16-B bank slots per lane group
// (conflict-free; scalar reads of one column over rows at pitch 260 were 4-way conflicts)
#define EW_ZP 260          // staged row pitch
#define EW_CP 68           // coefficient matrix pitch (narrow)
#define EW_CPW 132         // coefficient matrix pitch (wide, 128 candidates)
#define EW_GP 33           // Gram tile row pitch: the distance pass reads tiles transposed too

// DACP scratch of a workgroup: per-wave partial ranks and per-wave sorted-score tables
struct DacpBlockScratch {
  int rk[ECDA_THREADS / 64][TW_MAXB];   // [wave][row]: each wave's store is 64 consecutive ints
  float srt[ECDA_THREADS / 64][DAD_C][TW_MAXB];
};

// The DACP state a wave reads (uniform): tau, Q and the calibrated anchors.  Loaded by ONE
// unconditional load per lane (lane k < 20 holds dacp[k]) issued with the kernel's other entry
// loads, then broadcast by readlane: a load under a lane condition would be waited for on the
// spot (the compiler drains vmcnt where the paths merge), one memory round trip per value.
struct DacpState {
  float tau[DAD_C], Q[DAD_C], anc[DAD_C];
};

// segmented sums by DPP (no LDS-routed shuffles): the sum of each aligned group of N lanes lands
// in the group's LAST lane (N = 4, 8, 16 inside a 16-lane row; 32 adds row_bcast:15)
template <int N>
__device__ __forceinline__ float dpp_seg_sum(float v) {
  static_assert(N == 4 || N == 8 || N == 16 || N == 32, "segment");
  v += dad_dpp_f<0x111>(v);
  v += dad_dpp_f<0x112>(v);
  if constexpr (N >= 8) v += dad_dpp_f<0x114>(v);
  if constexpr (N >= 16) v += dad_dpp_f<0x118>(v);
  if constexpr (N == 32) v += dad_dpp_f<0x142, 0xa>(v);
  return v;
}
__device__ __forceinline__ DacpState dacp_state_of(float dv) {
  DacpState d;
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) {
    d.tau[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), k));
    d.Q[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), 4 + k));
    d.anc[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), 16 + k));
  }
  return d;
}

// DACP thresholds (I/utils.py:449-507) by all 8 waves of a workgroup, every wave holding the
// scores s and pseudo-labels p of every noisy row (lane i = row i < Bn; p = -1 past Bn).  Wave g
// counts, for every row, the rows j in [8g, 8g + 8) of its class below it (ties by index:
// readlane sweep, bitwise so nothing branches); one barrier; the rank is the sum of the 8
// partials.  Then every wave sorts into its own table and lanes 0..3 take torch.quantile(linear)
// of their class (dacp_class_threshold, which the general path's dacp_thresholds calls too, so
// the thresholds and masks of the two paths are bit-identical); outputs uniform.
__device__ __forceinline__ void dacp_block8(const dad_config& cfg, int Bn, float s, int p, const DacpState& D,
                                            DacpBlockScratch& W, float (&tau)[DAD_C], float (&wc)[DAD_C],
                                            float (&that)[DAD_C], float (&fl)[DAD_C]) {
  const int lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  TAIL_STAMP_W1(7);
  int part = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int j = 8 * g + u;
    const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), j));
    const int pj = __builtin_amdgcn_readlane(p, j);
    part += (int)((pj == p) & ((sj < s) | ((sj == s) & (j < lane))));
  }
  W.rk[g][lane] = part;   // ([row][wave] put 8 rows of a store on one bank: 8-way conflicts)
  __syncthreads();
  int r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = W.rk[k][lane];
  const int cnt = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  TAIL_STAMP_W1(8);
  int ncls[DAD_C];
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) ncls[c] = (int)__popcll(__ballot(lane < Bn && p == c));
  float (*srt)[TW_MAXB] = W.srt[g];
  if (lane < Bn) srt[p][cnt] = s;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float tn = 0.0f, w = 0.0f, th = 0.0f, f = 0.0f;
  if (lane < DAD_C) {
    const int c = lane;
    dacp_class_threshold(cfg, c, sel4i(ncls, c), srt[c], D.Q, sel4(D.tau, c), sel4(D.anc, c), tn, w, th, f);
  }
  DAD_PROBE_FENCE2(tn, f);
  TAIL_STAMP_W1(9);
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    tau[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tn), c));
    wc[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), c));
    that[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(th), c));
    fl[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), c));
  }
  DAD_PROBE_FENCE2(tau[3], fl[3]);
  TAIL_STAMP_W1(10);
}

// the DACP / fixed-threshold mask of noisy row `lane` (I/train.py:413-420), score s, pseudo-label
// p; called by all 8 waves of a workgroup (one barrier inside when DACP is on)
struct WaveMask {
  float s, q[DAD_C];
  int p;                 // pseudo-label, -1 on lanes >= Bn
  bool m;                // masked in (confident)
  float tau[DAD_C], wc[DAD_C], that[DAD_C], fl[DAD_C];
};
__device__ __forceinline__ void block_mask(const dad_config& cfg, int Bn, const f32x4& zt, const DacpState& D,
                                           DacpBlockScratch& W, WaveMask& M) {
  const int lane = threadIdx.x & 63;
  {
    const float z[4] = {zt[0], zt[1], zt[2], zt[3]};
    teacher_certainty(z, cfg, M.q, M.s, M.p);   // every lane (rows past Bn are clamped copies)
  }
  if (lane >= Bn) {
    M.s = 0.0f;
    M.p = -1;
  }
  if (cfg.use_dacp) {
    dacp_block8(cfg, Bn, M.s, M.p, D, W, M.tau, M.wc, M.that, M.fl);
    M.m = (lane < Bn) & (M.s >= sel4(M.tau, M.p < 0 ? 0 : M.p));
  } else {
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) { M.tau[c] = 0.0f; M.wc[c] = 1.0f; M.that[c] = 0.0f; M.fl[c] = 0.0f; }
    M.m = (lane < Bn) & (M.s >= cfg.fixed_thr);
  }
}

struct TailW {
  DacpBlockScratch dw;
  double d[2][8];
  float f[2][4];
};

// The tail (block 0) for B, Bn <= 64: see tail_block (tail_general.hip) for the reference lines
// of each step.
// Every wave: entry loads, teacher certainty and the DACP mask (block_mask: one barrier);
// wave 0: CE on the clean logits (lane = clean row); wave 1: DACP outputs, epoch statistics and
// the masked KL (lane = noisy row); one barrier to combine.
__device__ __forceinline__ void tail_block_w(const DadTailArgs& a, TailW& T) {
  const dad_config& cfg = a.cfg;
  const int B = cfg.B, Bn = cfg.Bn;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* tf = a.tailf;
  float* extras = a.grad + DAD_NPARAM;
  const float eps = cfg.ls_eps;
  TAIL_STAMP(0);
  TAIL_CYCLES(12);
  // entry loads, unconditional (rows clamped): clean logits + labels, teacher and strong logits,
  // the DACP state
  const int rc = lane < B ? lane : B - 1, rn = lane < Bn ? lane : Bn - 1;
  const f32x4 zv = reinterpret_cast<const f32x4*>(a.logits)[rc];
  const int yv = (int)a.yc[rc];
  const f32x4 zt = reinterpret_cast<const f32x4*>(a.logits + (size_t)B * DAD_C)[rn];
  const f32x4 zs = reinterpret_cast<const f32x4*>(a.logits + (size_t)(B + Bn) * DAD_C)[rn];
  const float dv = a.dacp[lane < DAD_DACP_FLOATS ? lane : 0];
  // teacher probs + certainty + DACP mask (I/train.py:408-420, I/utils.py:400-507), lane = noisy row
  const DacpState D = dacp_state_of(dv);
  WaveMask M;
  block_mask(cfg, Bn, zt, D, T.dw, M);
  TAIL_STAMP_W1(4);
  if (w == 0) {
    // supervised CE with label smoothing on the clean logits (I/train.py:364,400), lane = row
    double ce_part = 0.0, b2p[4] = {0.0, 0.0, 0.0, 0.0};
    {
      const float z[4] = {zv[0], zv[1], zv[2], zv[3]};
      float lse, g[4];
      double loss;
      ce_row(z, yv, eps, B, lse, g, loss);
      for (int c = 0; c < 4; ++c) b2p[c] = lane < B ? (double)g[c] : 0.0;
      ce_part = lane < B ? loss : 0.0;
      if (lane < B) *reinterpret_cast<f32x4*>(a.gzb + (size_t)lane * DAD_C) = f32x4{g[0], g[1], g[2], g[3]};
    }
    const double ce = dad_wave_sum_d(ce_part) / (double)B;
    double b2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b2[c] = dad_wave_sum_d(b2p[c]);
    TAIL_STAMP(2);
    if (lane == 0) {
      T.d[0][0] = ce;
#pragma unroll
      for (int c = 0; c < 4; ++c) T.d[0][1 + c] = b2[c];
    }
  } else if (w == 1) {
    if (cfg.use_dacp) {
      if (lane < DAD_C) {
        const int c = lane;
        tf[DAD_T_W + c] = sel4(M.wc, c);
        tf[DAD_T_TAU_BEFORE + c] = sel4(D.tau, c);
        tf[DAD_T_TAU_AFTER + c] = sel4(M.tau, c);
        tf[DAD_T_FLOORED + c] = sel4(M.fl, c);
        tf[DAD_T_TAU_HAT + c] = sel4(M.that, c);
        extras[c] = sel4(M.fl, c);
      }
      // epoch statistics of update_class_quality_scores_epoch (I/utils.py:503-505)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double st = dad_wave_sum_d(M.p == c ? (double)M.s : 0.0);
        const double ct = dad_wave_sum_d(M.p == c ? 1.0 : 0.0);
        if (lane == 0) {
          extras[4 + c] = (float)st;
          extras[8 + c] = (float)ct;
        }
      }
    } else if (lane < DAD_C) {
      tf[DAD_T_W + lane] = 1.0f;
      extras[0 + lane] = 0.0f;
      extras[4 + lane] = 0.0f;
      extras[8 + lane] = 0.0f;
    }
    const float mk = M.m ? 1.0f : 0.0f;
    const float msum = (float)__popcll(__ballot(M.m));   // the mask sum (an exact count)
    const bool kl_on = msum > 1.0f;                      // I/train.py:444
    // masked consistency KL(q || p_student) (I/train.py:445-447) and its logit grad
    const float denom = msum + 1e-8f;
    double kl_part = 0.0, b2p[4] = {0.0, 0.0, 0.0, 0.0};
    {
      const float z[4] = {zs[0], zs[1], zs[2], zs[3]};
      float klb, g[4];
      kl_row(z, M.q, mk, kl_on, cfg.w_kl, denom, klb, g);
      for (int c = 0; c < 4; ++c) b2p[c] = lane < Bn ? (double)g[c] : 0.0;
      kl_part = lane < Bn ? (double)(klb * mk) : 0.0;
      if (lane < Bn) {
        *reinterpret_cast<f32x4*>(a.gzb + (size_t)(B + lane) * DAD_C) = f32x4{g[0], g[1], g[2], g[3]};
        // per-sample outputs (noisy batch) for inspection / ECDA
        tf[DAD_TAIL_HDR + lane] = M.s;
        tf[DAD_TAIL_HDR + Bn + lane] = (float)M.p;
        tf[DAD_TAIL_HDR + 2 * Bn + lane] = mk;
        *reinterpret_cast<f32x4*>(tf + DAD_TAIL_HDR + 3 * Bn + lane * 4) = f32x4{M.q[0], M.q[1], M.q[2], M.q[3]};
      }
    }
    TAIL_STAMP_W1(5);
    const double kls = dad_wave_sum_d(kl_part);
    double b2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) b2[c] = dad_wave_sum_d(b2p[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) T.d[1][1 + c] = b2[c];
      T.f[1][0] = kl_on ? (float)(kls / (double)denom) : 0.0f;
      T.f[1][1] = msum;
      T.f[1][2] = kl_on ? 1.0f : 0.0f;
    }
    TAIL_STAMP_W1(6);
  }
  __syncthreads();
  if (tid == 0) {
    const float kl_on = T.f[1][2];
    tf[DAD_T_CE] = (float)T.d[0][0];
    tf[DAD_T_KL] = T.f[1][0];
    tf[DAD_T_SCL] = 0.0f;
    tf[DAD_T_MSUM] = T.f[1][1];
    tf[DAD_T_KL_ON] = kl_on;
    tf[DAD_T_ECDA_ON] = (kl_on != 0.0f && cfg.ecda_on) ? 1.0f : 0.0f;
  }
  if (tid < 4) a.grad[DAD_OFF_B2 + tid] = (float)(T.d[0][1 + tid] + T.d[1][1 + tid]);
  TAIL_CYCLES(13);
  TAIL_STAMP(1);
}

struct __attribute__((aligned(16))) EcdaW {
  union {
    float zc[(TW_MAXB + 1) * EW_ZP];    // narrow (<= 64 candidates): staged candidate rows + a spare row
    float dbw[2 * TW_MAXB * EW_CPW];    // wide (65..128): D, then the MMD coefficients
  } a;
  union {
    DacpBlockScratch dw;                     // DACP scratch (before barrier 1)
    float gp[10][32 * EW_GP];                // Gram partial tiles (after barrier 1)
  } b;
  union {
    float cp[ECDA_THREADS / 64][DAD_C][DAD_H];   // per-wave centroid partial sums (until barrier 2)
    float dbn[TW_MAXB * EW_CP];                  // narrow: D, then the MMD coefficients (after barrier 2)
  } c;
  float cent[DAD_C][DAD_H];
  float nz[2 * TW_MAXB], wz[2 * TW_MAXB], rs[2 * TW_MAXB];
  int rowz[2 * TW_MAXB], mem[2 * TW_MAXB];
  int cnt[DAD_C];                       // masked noisy rows per class (pseudo-label)
  float pd[DAD_C][DAD_C];
  float msp[ECDA_THREADS / 64][DAD_H];   // per-wave sums of the member rows minus candidate row 0
  double nsp[ECDA_THREADS / 64];        // per-wave sums of |member row - candidate row 0|^2
  double t3p[ECDA_THREADS / 64][3];
  float cmp[ECDA_THREADS / 64];
};

// upper-triangle tile pair index of (ti <= tj) among nt tiles, and its inverse
__device__ __forceinline__ int ew_pair(int ti, int tj, int nt) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }
__device__ __forceinline__ void ew_pair_inv(int pr, int nt, int& ti, int& tj) {
  ti = 0;
  while (pr >= nt - ti) { pr -= nt - ti; ++ti; }
  tj = ti + pr;
}

// Member gradients of a narrow class (NP = 32 or 64 padded candidates, rows and coefficients in
// LDS): 2 (rs_i z_i - (Csym Z)_i) scaled, plus the compactness and repulsion parts of the noisy
// members, per item of 32 candidates x 32 hidden units.  Every LDS operand of an item -- the
// NP/8 coefficient reads and 4 NP/8 row reads of the MFMA chain and the 16 rows' epilogue values
// -- is issued before its first MFMA.  The 32 x 32 result goes out through the wave's own LDS
// tile (the dead Gram partials, pitch EW_TP: the two lane halves' rows 32 banks apart), read back
// as 4 consecutive hidden units per lane: 4 dwordx4 stores per lane instead of 16 dword stores
// (the phase was bound by issuing the 32 KB of stores, not by the MFMA chain).
#define EW_TP 40
static_assert(ECDA_NG * 32 * EW_TP <= sizeof(EcdaW::b) / sizeof(float), "ew_member_grads: a 32 x EW_TP tile per wave in S.b");
// NK: the 8-candidate blocks of the (Csym Z) chain, ceil(ncand_all / 8) (the coefficients and rows
// past the candidates are zero, so the blocks they fill add nothing): a 33-candidate class runs 5
// blocks of its 64-row tiling's 8
// 64-row tiling: the 8-candidate column blocks of the coefficient matrix that the member-gradient
// chain reads (ew_member_grads<64, NK> reads columns [0, 8 NK) of db) and that the coefficient pass
// therefore writes: ONE helper for both, so the pass never leaves a read column stale
__device__ __forceinline__ int ew_nk64(int ncand_all) { return max((ncand_all + 7) >> 3, 5); }

template <int NP, int NK, class RG>
__device__ __forceinline__ void ew_member_grads(EcdaW& S, const float* db, int dp, int c, int ncs, int ncand_all,
                                                float mmd_scale, float comp_scale, float* ge_c, float* ge_s,
                                                float* sink, const RG& repg_at) {
  static_assert(NK >= 1 && NK <= NP / 8, "ew_member_grads: NK 8-candidate blocks of NP");
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = lane >> 5, l32 = lane & 31;
  for (int item = g; item < (NP / 32) * (DAD_H / 32); item += ECDA_NG) {
    const int ti = item >> 3, tc = item & 7;
    const int d = 32 * tc + l32;
    const float* ra = &db[(32 * ti + l32) * dp + 4 * kh];
    f32x4 av[NK];
    float bv[NK][4];
#pragma unroll
    for (int q = 0; q < NK; ++q) {
      av[q] = *reinterpret_cast<const f32x4*>(ra + 8 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[q][e] = S.a.zc[(8 * q + 4 * kh + e) * EW_ZP + d];
    }
    float zi[16], rsv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 32 * ti + dad_acc_row(r, kh);   // (< NP <= TW_MAXB: staged or zero row)
      const int ic = i < ncand_all ? i : 0;
      zi[r] = S.a.zc[i * EW_ZP + d];
      rsv[r] = S.rs[ic];
    }
    const float mu = S.cent[c][d], rg = repg_at(d);
    f32x16 acc = f32x16{};
#pragma unroll
    for (int q = 0; q < NK; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][e], bv[q][e], acc, 0, 0, 0);
    ECDA_CYC(25);
    float* stg = &S.b.gp[0][0] + g * (32 * EW_TP);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 32 * ti + dad_acc_row(r, kh);
      const bool noisy = i >= ncs;
      stg[dad_acc_row(r, kh) * EW_TP + l32] =
          mmd_scale * (2.0f * (rsv[r] * zi[r] - acc[r])) + (noisy ? comp_scale * (zi[r] - mu) + rg : 0.0f);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the wave's own tile: LDS ops are in order)
    ECDA_CYC(26);
    // every row stored: members to their ge row, the rest to the sink (no branch)
    const int rl = lane >> 3, c4 = 4 * (lane & 7);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = rl + 8 * k, i = 32 * ti + row;
      const int ic = i < ncand_all ? i : 0;
      const bool mem = (i < ncand_all) & (S.mem[ic] != 0);
      const f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * EW_TP + c4);
      float* dst = mem ? (i >= ncs ? ge_s : ge_c) + (size_t)S.rowz[ic] * DAD_H + 32 * tc + c4 : sink + 32 * tc + c4;
      *reinterpret_cast<f32x4*>(dst) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // tile reads done before the next item's writes
    ECDA_CYC(27);
  }
}

// The class work after the candidates are known.  WIDE = more than 64 candidates: rows are read
// from the embedding buffer (global, through the candidate -> row table) instead of LDS.
template <bool WIDE>
__device__ __forceinline__ void ecda_class_w(const DadEcdaArgs& a, const int c, EcdaW& S, const WaveMask& M,
                                             const f32x4 (&ps)[ECDA_PRE_U], const int prd,
                                             const int ncls, const int nvalid, const int npairs, const bool gc,
                                             const bool rep_on, const float rep_coef, const float att_c, const int ncs,
                                             const int ncand_all, const double wsum_t) {
  const dad_config& cfg = a.cfg;
  const int B = cfg.B, Bn = cfg.Bn;
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = lane >> 5, l32 = lane & 31;
  const float* emb_c = a.emb;
  const float* emb_s = a.emb + (size_t)(B + Bn) * DAD_H;
  const int npad = ncand_all <= 32 ? 32 : (ncand_all <= 64 ? 64 : 128);
  const int nt = npad / 32;                       // 32-row tiles
  const int npt = nt * (nt + 1) / 2;              // upper-triangle tile pairs: 1, 3 or 10
  const int ks = npt == 1 ? 8 : (npt == 3 ? 2 : 1);   // K splits per pair
  float* db = WIDE ? S.a.dbw : S.c.dbn;
  const int dp = WIDE ? EW_CPW : EW_CP;
  const int cnc = S.cnt[c];
  const int nmem = ncs + cnc;   // members: clean candidates + masked noisy candidates
  // candidate row i: LDS (narrow) or the embedding buffer (wide; rows past the candidates: zero)
  auto rowp = [&](int i) -> const float* {
    if constexpr (WIDE) return (i < ncs ? emb_c : emb_s) + (size_t)S.rowz[i < ncand_all ? i : 0] * DAD_H;
    else return &S.a.zc[i * EW_ZP];
  };
  auto rowv = [&](int i, int col) -> float {
    if constexpr (WIDE) return i < ncand_all ? rowp(i)[col] : 0.0f;
    else return S.a.zc[i * EW_ZP + col];
  };
  if (gc) {
    // squared norms of the candidate rows (a runtime loop: only the candidates are summed), and
    // for the bandwidth this wave's sums over its member rows of d = z - z0 and |d|^2, z0 =
    // candidate row 0 (lane = 4 hidden units).  Post-ReLU embeddings share a large positive mean;
    // centred on a row of the class, the identity below sums no large cancelling terms.
    f32x4 ms = f32x4{};
    double ns = 0.0;
    const f32x4 z0 = *reinterpret_cast<const f32x4*>(rowp(0) + 4 * lane);
    for (int r = g; r < ncand_all; r += ECDA_NG) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(rowp(r) + 4 * lane);
      const float nr = dad_wave_sum(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
      if (lane == 0) S.nz[r] = nr;
      if (S.mem[r]) {
        const f32x4 d = v - z0;
        ms += d;
        ns += (double)dad_wave_sum(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]);
      }
    }
    *reinterpret_cast<f32x4*>(&S.msp[g][4 * lane]) = ms;
    if (lane == 0) S.nsp[g] = ns;
    // Gram partials: tile pair (ti, tj) over a K slice, fp32 matrix cores.  The 64-row tiling
    // (3 pairs) cuts pairs (0,0) and (0,1) into 4 slices and (1,1) into 2: 10 items in the 10
    // partial slots, dealt so that the waves w and w + 4 (one SIMD's pair) hold 6 slices' MFMAs
    // each (3 x 64 or 128 + 64 of K) instead of two 128-K items on two SIMDs and one on the others
    for (int item = g; item < (npt == 3 ? 10 : npt * ks); item += ECDA_NG) {
      int pr, sl, nsl;
      if (npt == 3) {
        // item -> pair (2 bits) | slice (2 bits): 0:(0,2) 1:(1,1) 2:(2,0) 3:(2,1) 4:(0,3) 5:(1,2)
        // 6:(0,0) 7:(0,1) 8:(1,0) 9:(1,3)
        constexpr uint64_t kDeal = 0x2ull | (0x5ull << 4) | (0x8ull << 8) | (0x9ull << 12) | (0x3ull << 16) |
                                   (0x6ull << 20) | (0x0ull << 24) | (0x1ull << 28) | (0x4ull << 32) | (0x7ull << 36);
        const int v = (int)((kDeal >> (4 * item)) & 15u);
        pr = v >> 2;
        sl = v & 3;
        nsl = pr < 2 ? 4 : 2;
      } else {
        pr = item / ks;
        sl = item - pr * ks;
        nsl = ks;
      }
      const int slot = npt == 3 ? (pr < 2 ? 4 * pr : 8) + sl : item;
      int ti, tj;
      ew_pair_inv(pr, nt, ti, tj);
      const int kw = DAD_H / nsl, k0 = sl * kw;
      const int ia = 32 * ti + l32, ib = 32 * tj + l32;
      // MFMA step e of a k-block of 8 takes k-index k + 4 kh + e on both operands (any k order
      // sums the same dot products): each lane reads 4 consecutive floats per operand
      const float* ra = rowp(ia) + 4 * kh;
      const float* rb = rowp(ib) + 4 * kh;
      const bool za = WIDE && ia >= ncand_all, zb = WIDE && ib >= ncand_all;
      f32x16 acc = f32x16{};
      for (int k = k0; k < k0 + kw; k += 8) {
        f32x4 av = *reinterpret_cast<const f32x4*>(ra + k), bv = *reinterpret_cast<const f32x4*>(rb + k);
        if (za) av = f32x4{};
        if (zb) bv = f32x4{};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) S.b.gp[slot][dad_acc_row(r, kh) * EW_GP + l32] = acc[r];
    }
  }
  // centroids of every class over its masked noisy rows, partials combined in wave order
  for (int e = tid; e < DAD_C * DAD_H; e += ECDA_THREADS) {
    const int k = e >> 8, hh = e & (DAD_H - 1);
    float sk = 0.0f;
#pragma unroll
    for (int gg = 0; gg < ECDA_NG; ++gg) sk += S.c.cp[gg][k][hh];
    const int nk = S.cnt[k];
    S.cent[k][hh] = nk > 0 ? sk / (float)nk : 0.0f;
  }
  ECDA_STAMP(4);
  __syncthreads();   // ---------------------------------------------------------------- 2
  ECDA_STAMP(5);
  ECDA_CYC(6);
  // element ownership of the [npad x npad] matrices: row ei, columns ej0 .. ej0 + ept - 1
  const int ept = npad * npad / ECDA_THREADS;     // 2, 8 or 32
  const int tpr = npad / ept;                     // threads per row: 16, 8 or 4
  const int ei = tid / tpr, ej0 = (tid - ei * tpr) * ept;
  // centroid distances (I/utils.py:582-595): 32 threads per (p, q) pair, pair-symmetric order
  {
    const int pair = tid / 32, t32 = tid & 31;
    float d = 0.0f;
    if (pair < DAD_C * DAD_C) {
      const int p = pair / DAD_C, q = pair % DAD_C;
      const int lo = p < q ? p : q, hi = p < q ? q : p;
      const int np = S.cnt[p];
      const int nq = S.cnt[q];
      if (p < ncls && q < ncls && np > 0 && nq > 0 && p != q) {
        const f32x4* a0 = reinterpret_cast<const f32x4*>(&S.cent[lo][t32 * (DAD_H / 32)]);
        const f32x4* a1 = reinterpret_cast<const f32x4*>(&S.cent[hi][t32 * (DAD_H / 32)]);
        const f32x4 x0 = a0[0], x1 = a0[1], y0 = a1[0], y1 = a1[1];
        const float v[8] = {x0[0] - y0[0], x0[1] - y0[1], x0[2] - y0[2], x0[3] - y0[3],
                            x1[0] - y1[0], x1[1] - y1[1], x1[2] - y1[2], x1[3] - y1[3]};
#pragma unroll
        for (int k = 0; k < 8; ++k) d += v[k] * v[k];
      }
    }
    d = dpp_seg_sum<32>(d);
    if (pair < DAD_C * DAD_C && t32 == 31) S.pd[pair / DAD_C][pair % DAD_C] = sqrtf(d);
  }
  ECDA_CYC(20);
  const float Wss = (float)ncs * (float)ncs + 1e-8f;
  const float Wtt = (float)(wsum_t * wsum_t) + 1e-8f;
  const float Wst = (float)((double)ncs * wsum_t) + 1e-8f;
  if (gc) {
    // compactness partial (I/utils.py:614-616): this wave's masked noisy rows of class c
    float cpart = 0.0f;
    const f32x4 mu = *reinterpret_cast<const f32x4*>(&S.cent[c][4 * lane]);
#pragma unroll
    for (int u = 0; u < ECDA_PRE_U; ++u) {
      const int b = g + ECDA_NG * u;
      const int pk = __builtin_amdgcn_readlane(prd, b < 64 ? b : 0);
      if (b < Bn && pk == c) {
        const f32x4 df = ps[u] - mu;
        cpart += ((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]) + df[3] * df[3];
      }
    }
    cpart = dad_wave_sum(cpart);
    // detached bandwidth (I/utils.py:538-544) without the distance matrix: over the nmem member
    // rows, with d_i = z_i - z0 for any fixed z0, sum_ij |z_i - z_j|^2 = 2 nmem sum_i |d_i|^2 -
    // 2 |sum_i d_i|^2, from the waves' partial sums (every wave alike, combined in double), so the
    // kernel values and coefficients follow the distances in the same pass (the distance matrix
    // no longer makes a round trip through LDS and a barrier before them)
    f32x4 m = f32x4{};
#pragma unroll
    for (int gg = 0; gg < ECDA_NG; ++gg) m += *reinterpret_cast<const f32x4*>(&S.msp[gg][4 * lane]);
    const double msq = dad_wave_sum_d(((double)m[0] * m[0] + (double)m[1] * m[1]) + ((double)m[2] * m[2] + (double)m[3] * m[3]));
    double nsq = 0.0;
#pragma unroll
    for (int gg = 0; gg < ECDA_NG; ++gg) nsq += S.nsp[gg];
    const double bws = fmax(2.0 * (double)nmem * nsq - 2.0 * msq, 0.0);
    float bw = nmem > 1 ? (float)(bws / (double)(nmem * nmem - nmem)) : 1.0f;
    bw = bw / 4.0f;
    float ibw[5];
#pragma unroll
    for (int mm = 0; mm < 5; ++mm) ibw[mm] = 1.0f / (bw * (float)(1 << mm) + 1e-8f);
    ECDA_CYC(21);
    // the weighted kernel terms (I/utils.py:546-563): every ordered member pair (i, j); the
    // symmetric coefficients Csym_ij = dmmd/dD_ij + dmmd/dD_ji; branch-free, invalid elements 0
    double t3[3] = {0.0, 0.0, 0.0};
    float rsp = 0.0f;
    const int ic = ei < ncand_all ? ei : 0;
    const bool mi = (ei < ncand_all) & (S.mem[ic] != 0);
    const float wi = S.wz[ic];
    const bool si = ei < ncs;
    const float css = 2.0f / Wss, ctt = 2.0f / Wtt, cst = -2.0f / Wst;
    auto coef = [&](const int j) {
      const int i = ei;
      // G_ij read at (min, max) in the upper-triangle tiles: D is symmetric bit for bit
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      const int pr = ew_pair(lo >> 5, hi >> 5, nt);
      float gsum = 0.0f;
      const int sb = npt == 3 ? (pr < 2 ? 4 * pr : 8) : pr * ks, sn = npt == 3 ? (pr < 2 ? 4 : 2) : ks;
      for (int s2 = 0; s2 < sn; ++s2) gsum += S.b.gp[sb + s2][(lo & 31) * EW_GP + (hi & 31)];
      const bool ok = (i < ncand_all) & (j < ncand_all) & (i != j);
      const float d = ok ? fmaxf((S.nz[lo] + S.nz[hi]) - 2.0f * gsum, 0.0f) : 0.0f;
      const int jc = j < ncand_all ? j : 0;
      const bool on = mi & (j < ncand_all) & (S.mem[jc] != 0);
      const float wj = S.wz[jc];
      float K = 0.0f, dK = 0.0f;
#pragma unroll
      for (int mm = 0; mm < 5; ++mm) {
        const float ex = __expf(-d * ibw[mm]);
        K += ex;
        dK -= ex * ibw[mm];
      }
      const bool sj = j < ncs;
      const bool ss = on & si & sj, tt = on & !si & !sj, st = on & si & !sj, ts = on & !si & sj;
      const float ww = wi * wj;
      t3[0] += ss ? (double)K : 0.0;
      t3[1] += tt ? (double)K * ww : 0.0;
      t3[2] += st ? (double)K * wj : 0.0;
      // Csym: SS 2/Wss dK, TT 2 w_i w_j/Wtt dK, ST -2 w_j/Wst dK, TS -2 w_i/Wst dK
      const float vss = css * dK, vtt = (ctt * ww) * dK, vst = (cst * wj) * dK, vts = (cst * wi) * dK;
      float v = ss ? vss : (tt ? vtt : (st ? vst : (ts ? vts : 0.0f)));
      v = i == j ? 0.0f : v;
      rsp += v;
      return v;
    };
    // 64-row tiling: the thread's 8 elements unrolled, their stores after the last one (a store
    // to db inside the loop kept the next element's LDS reads behind it: pairs 9.7k -> 8.9k
    // cycles for a 38-41 member class; the 32-row case, 2 elements, measured no better so)
    if (!WIDE && npad == 64) {
      // the 64-row tiling: thread column jt + tpr e, only the columns the member-gradient chain
      // reads (8 ceil(ncand / 8), ew_member_grads' NK blocks), so a 40-candidate class runs 5 of
      // the 8 elements per thread; rows past the candidates get their zeros without the kernel math
      const int jt = ej0 / ept, kz = 8 * ew_nk64(ncand_all);   // = ew_member_grads' 8 NK columns
      float v8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = jt + 8 * e;
        v8[e] = (j < kz && ei < ncand_all) ? coef(j) : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (jt + 8 * e < kz) db[ei * dp + jt + 8 * e] = v8[e];
    } else {
      for (int e = 0; e < ept; ++e) db[ei * dp + ej0 + e] = coef(ej0 + e);
    }
    ECDA_CYC(22);
    // row sums of the coefficients: the tpr threads of a row are adjacent lanes
    rsp = tpr == 16 ? dpp_seg_sum<16>(rsp) : (tpr == 8 ? dpp_seg_sum<8>(rsp) : dpp_seg_sum<4>(rsp));
    if ((tid & (tpr - 1)) == tpr - 1) S.rs[ei] = rsp;
#pragma unroll
    for (int k = 0; k < 3; ++k) t3[k] = dad_wave_sum_d(t3[k]);
    if (lane == 0) { S.t3p[g][0] = t3[0]; S.t3p[g][1] = t3[1]; S.t3p[g][2] = t3[2]; S.cmp[g] = cpart; }
    ECDA_CYC(23);
  }
  __syncthreads();   // ---------------------------------------------------------------- 3
  ECDA_STAMP(7);
  const float wscale = cfg.w_ecda;
  float pd[DAD_C][DAD_C];
#pragma unroll
  for (int p = 0; p < DAD_C; ++p)
#pragma unroll
    for (int q = 0; q < DAD_C; ++q) pd[p][q] = S.pd[p][q];
  float rep = 0.0f;
  if (nvalid > 1) {
    float sp = 0.0f;
#pragma unroll
    for (int p = 0; p < DAD_C; ++p)
#pragma unroll
      for (int q = p + 1; q < DAD_C; ++q) {
        const int np = S.cnt[p];
        const int nq = S.cnt[q];
        if (q < ncls && np > 0 && nq > 0) sp += pd[p][q];
      }
    rep = -sp / (float)npairs;
  }
  // repulsion grad of the class's noisy members at hidden unit d (d rep / d mu_c / n_c), each
  // lane for its own columns: rk * sum_q (cent_c[d] - cent_q[d]) / pd_cq over the valid other
  // classes in the reference's class order; the reciprocals are wave-uniform, taken once
  float rq[DAD_C];
#pragma unroll
  for (int q = 0; q < DAD_C; ++q) {
    const int nq = S.cnt[q];
    const float nd = S.pd[c][q];
    rq[q] = (rep_on && q != c && q < ncls && nq > 0 && nd > 0.0f) ? 1.0f / nd : 0.0f;
  }
  const float rk = rep_on ? -wscale * rep_coef / (float)npairs / (float)cnc : 0.0f;
  auto repg_at = [&](int d) -> float {
    if (!rep_on) return 0.0f;
    const float cc0 = S.cent[c][d];
    float gsum = 0.0f;
#pragma unroll
    for (int q = 0; q < DAD_C; ++q) gsum += rq[q] != 0.0f ? (cc0 - S.cent[q][d]) * rq[q] : 0.0f;
    return rk * gsum;
  };
  float* ge_c = a.ge;
  float* ge_s = a.ge + (size_t)B * DAD_H;
  if (gc) {
    double t3[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int gg = 0; gg < ECDA_NG; ++gg) {
      t3[0] += S.t3p[gg][0];
      t3[1] += S.t3p[gg][1];
      t3[2] += S.t3p[gg][2];
    }
    // t_ss, t_tt, t_st as the reference forms them in float32 (I/utils.py:558-563)
    const float mmd = (float)t3[0] / Wss + (float)t3[1] / Wtt - 2.0f * ((float)t3[2] / Wst);
    float csum = 0.0f;
#pragma unroll
    for (int gg = 0; gg < ECDA_NG; ++gg) csum += S.cmp[gg];
    const float comp = csum / (float)cnc;
    if (tid == 0) {
      a.tail_terms[c] = att_c * (mmd + cfg.ecda_gamma * comp + cfg.ecda_delta * rep);
      a.tail_terms[DAD_T_ECDA_GATE - DAD_T_ECDA_TERM + c] = 1.0f;
    }
    ECDA_CYC(24);
    const float mmd_scale = wscale * att_c;
    const float comp_scale = wscale * att_c * cfg.ecda_gamma * (2.0f / (float)cnc);
    // member grads 2 sum_j Csym_ij (z_i - z_j) = 2 (rs_i z_i - (Csym Z)_i): (Csym Z) on the
    // matrix cores, 32 candidates x 32 hidden units per item
    if constexpr (!WIDE) {
      if (npad == 32) {
        ew_member_grads<32, 4>(S, db, dp, c, ncs, ncand_all, mmd_scale, comp_scale, ge_c, ge_s, a.sink, repg_at);
      } else {
        const int nk = ew_nk64(ncand_all);   // 5 .. 8 (33 .. 64 candidates): the columns the pass wrote
        if (nk <= 5) ew_member_grads<64, 5>(S, db, dp, c, ncs, ncand_all, mmd_scale, comp_scale, ge_c, ge_s, a.sink, repg_at);
        else if (nk == 6) ew_member_grads<64, 6>(S, db, dp, c, ncs, ncand_all, mmd_scale, comp_scale, ge_c, ge_s, a.sink, repg_at);
        else if (nk == 7) ew_member_grads<64, 7>(S, db, dp, c, ncs, ncand_all, mmd_scale, comp_scale, ge_c, ge_s, a.sink, repg_at);
        else ew_member_grads<64, 8>(S, db, dp, c, ncs, ncand_all, mmd_scale, comp_scale, ge_c, ge_s, a.sink, repg_at);
      }
    }
    for (int item = g; WIDE && item < nt * (DAD_H / 32); item += ECDA_NG) {
      const int ti = item >> 3, tc = item & 7;
      const int d = 32 * tc + l32;
      f32x16 acc = f32x16{};
      const float* ra = &db[(32 * ti + l32) * dp + 4 * kh];
      for (int k = 0; k < npad; k += 8) {
        // step e: candidate k + 4 kh + e (one b128 read of the coefficient row per lane)
        const f32x4 av = *reinterpret_cast<const f32x4*>(ra + k);
        float bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = rowv(k + 4 * kh + e, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
      }
      const float mu = S.cent[c][d], rg = repg_at(d);
      // every accumulator row stored: members to their ge row, the rest to the sink (no branch)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = 32 * ti + dad_acc_row(r, kh);
        const int ic = i < ncand_all ? i : 0;
        const bool ok = (i < ncand_all) & (S.mem[ic] != 0);
        const float zi = rowv(i, d);
        const bool noisy = i >= ncs;
        const float gv = mmd_scale * (2.0f * (S.rs[ic] * zi - acc[r])) + (noisy ? comp_scale * (zi - mu) + rg : 0.0f);
        float* dst = ok ? (noisy ? ge_s : ge_c) + (size_t)S.rowz[ic] * DAD_H + d : a.sink + d;
        *dst = gv;
      }
    }
  } else {
    // a class below the gate only feeds the repulsion: its noisy members get repg
    const int nct = ncand_all - ncs;
    for (int e = tid; e < nct * (DAD_H / 4); e += ECDA_THREADS) {
      const int i = ncs + e / (DAD_H / 4), q = e % (DAD_H / 4);
      if (S.mem[i]) {
        const f32x4 v = f32x4{repg_at(4 * q), repg_at(4 * q + 1), repg_at(4 * q + 2), repg_at(4 * q + 3)};
        reinterpret_cast<f32x4*>(ge_s + (size_t)S.rowz[i] * DAD_H)[q] = v;
      }
    }
  }
  for (int i = tid; i < ncand_all; i += ECDA_THREADS)
    if (S.mem[i]) a.eflag[i < ncs ? S.rowz[i] : B + S.rowz[i]] = 1u;
  ECDA_STAMP(8);
  if (tid == 0) ECDA_STAMP_SIZES(c, ncand_all, ncs);
}

// One ECDA class (I/utils.py:565-632, class-aware) for B, Bn <= 64.
__device__ __forceinline__ void ecda_block_w(const DadEcdaArgs& a, const DadTailArgs& ta, const int c, EcdaW& S) {
  const dad_config& cfg = a.cfg;
  const int B = cfg.B, Bn = cfg.Bn;
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* emb_c = a.emb;
  const float* emb_s = a.emb + (size_t)(B + Bn) * DAD_H;
  ECDA_STAMP(0);
  // ---- entry: teacher logits (lane = noisy row), labels (lane = clean row), and the embedding
  // rows this wave handles (rows g, g + 8, ...; lane = 16-B column chunk), all in flight
  // every load unconditional (rows clamped; the clamped duplicates are never used): a load
  // under a condition is waited for where the paths merge, one round trip each
  const int rc = lane < B ? lane : B - 1, rn = lane < Bn ? lane : Bn - 1;
  const f32x4 zt = reinterpret_cast<const f32x4*>(ta.logits + (size_t)B * DAD_C)[rn];
  const int yv = (int)a.yc[rc];
  const float dv = ta.dacp[lane < DAD_DACP_FLOATS ? lane : 0];
  // the rows are issued after the DACP inputs, so the DACP waits for those alone (counted
  // vmcnt) while the rows are still in flight
  __builtin_amdgcn_sched_barrier(0);
  // strong rows: all (the centroids of every class need the masked ones)
  f32x4 pc[ECDA_PRE_U], ps[ECDA_PRE_U];
#pragma unroll
  for (int u = 0; u < ECDA_PRE_U; ++u) {
    const int b = g + ECDA_NG * u;
    ps[u] = reinterpret_cast<const f32x4*>(emb_s + (size_t)(b < Bn ? b : Bn - 1) * DAD_H)[lane];
  }
  const int y = lane < B ? yv : -1;
  // clean rows: only this class's candidates (label c), compacted; wave g loads candidates
  // g, g + 8, ... (row 0 past the last), in flight during the DACP.  Per-CU load bandwidth from
  // another XCD's writes is the limit here, so rows nobody stages are not fetched.
  const uint64_t bcl = __ballot(y == c);
  const int ncl = (int)__popcll(bcl);
  const int posl = (int)__popcll(bcl & ((1ull << lane) - 1ull));
#pragma unroll
  for (int u = 0; u < ECDA_PRE_U; ++u) {
    const int j = g + ECDA_NG * u;
    const uint64_t hit = __ballot((y == c) & (posl == j));
    const int row = hit ? (int)__builtin_ctzll(hit) : 0;
    pc[u] = reinterpret_cast<const f32x4*>(emb_c + (size_t)row * DAD_H)[lane];
  }
  // ---- the DACP mask, in this wave (every wave computes the same one)
  WaveMask M;
  block_mask(cfg, Bn, zt, dacp_state_of(dv), S.b.dw, M);
  ECDA_STAMP(1);
  const int prd = M.m ? M.p : -1;                                // I/utils.py:573-576
  const float msum = (float)__popcll(__ballot(M.m));
  if (!(msum > 1.0f && cfg.ecda_on)) return;                     // I/train.py:444,450
  const int ncls = cfg.use_dacp ? DAD_C : (Bn < DAD_C ? Bn : DAD_C);
  if (c >= ncls) return;
  // per-class counts, attention, gates, repulsion coefficient (uniform; I/utils.py:582-610)
  int cc[DAD_C], cn[DAD_C];
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) {
    cc[k] = k < ncls ? (int)__popcll(__ballot(y == k)) : 0;
    cn[k] = k < ncls ? (int)__popcll(__ballot(prd == k)) : 0;
  }
  float att[DAD_C];
  if (cfg.use_dacp) {
    const float wmean = (((M.wc[0] + M.wc[1]) + M.wc[2]) + M.wc[3]) / 4.0f;
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) att[k] = expf(cfg.ecda_att_lambda * (wmean - M.wc[k]));
  } else {
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) att[k] = 1.0f;
  }
  int nvalid = 0;
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) nvalid += (k < ncls && cn[k] > 0) ? 1 : 0;
  const int npairs = nvalid * (nvalid - 1) / 2;
#if DAD_PROBE_ON
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stamps build: when the prefetched rows have landed
  ECDA_STAMP(9);
  ECDA_CYC(19);
#endif
  bool gated[DAD_C];
  float rep_coef = 0.0f;
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) {
    gated[k] = k < ncls && cc[k] >= 2 && cn[k] >= 2;   // I/utils.py:609-610
    if (gated[k]) rep_coef += att[k] * cfg.ecda_delta;
  }
  const int cnc = c == 0 ? cn[0] : (c == 1 ? cn[1] : (c == 2 ? cn[2] : cn[3]));
  const int ccc = c == 0 ? cc[0] : (c == 1 ? cc[1] : (c == 2 ? cc[2] : cc[3]));
  const bool gc = c == 0 ? gated[0] : (c == 1 ? gated[1] : (c == 2 ? gated[2] : gated[3]));
  const float att_c = sel4(att, c);
  const bool rep_on = nvalid > 1 && cnc > 0 && rep_coef != 0.0f;
  ECDA_CYC(13);
  if (!gc && !rep_on) return;
  // candidates: clean rows of label c (members when gated), then the noisy rows of pseudo-label c
  // that the mask takes in (I/utils.py:573-576, the reference's target set); positions by ballot
  // prefix counts, every wave alike.  Noisy rows of pseudo-label c left out by the mask take no part
  // in any term (kernel pairs, bandwidth, centroids, gradients), so they are not staged: a teacher
  // that sends most of the noisy batch to one class with half of it masked out no longer pushes
  // that class past 64 candidates into the wide path
  const bool ccand = gc && y == c;
  const bool ncand = lane < Bn && M.p == c && M.m;
  const uint64_t bc = __ballot(ccand), bn = __ballot(ncand);
  const int ncs = gc ? ccc : 0;
  const int ncand_all = ncs + (int)__popcll(bn);
  const bool wide = ncand_all > TW_MAXB;
  const uint64_t below = (1ull << lane) - 1ull;
  const int posc = (int)__popcll(bc & below);
  const int posn = ncs + (int)__popcll(bn & below);
  // ---- stage: candidate norms (and, narrow, rows), weights, rows and member flags; the
  // per-wave centroid partial sums of every class
  // a wave's candidate rows: their candidate positions (uniform), the others go to the spare
  // row TW_MAXB (narrow) -- unconditional stores, no branches; norms by one batched butterfly
  int npos[2 * ECDA_PRE_U];
#pragma unroll
  for (int u = 0; u < ECDA_PRE_U; ++u) {
    const int b = g + ECDA_NG * u;                 // noisy row b; clean candidate b (compacted)
    const bool okc = gc & (b < ncl);
    const bool okn = (b < Bn) & (((bn >> b) & 1ull) != 0);
    npos[2 * u] = __builtin_amdgcn_readfirstlane(okc ? b : -1);
    npos[2 * u + 1] = __builtin_amdgcn_readfirstlane(okn ? __builtin_amdgcn_readlane(posn, b) : -1);
    // candidate rows only, under uniform (scalar) branches: storing every row (the others to a
    // spare row) had all 8 waves queue 128 KB of LDS writes at once (~2500 cycles per wave)
    if (!wide & okc) *reinterpret_cast<f32x4*>(&S.a.zc[npos[2 * u] * EW_ZP + 4 * lane]) = pc[u];
    if (!wide & okn) *reinterpret_cast<f32x4*>(&S.a.zc[npos[2 * u + 1] * EW_ZP + 4 * lane]) = ps[u];
  }
  ECDA_CYC(14);
  // (the candidates' squared norms are taken from the staged rows after barrier 1: here the
  // compiler computed the wave sums of all 16 rows, candidate or not, ~2000 cycles)
  ECDA_STAMP(12);
  ECDA_CYC(15);
  if (!wide) {
    const int npad = ncand_all <= 32 ? 32 : 64;
    for (int r = ncand_all + g; r < npad; r += ECDA_NG) *reinterpret_cast<f32x4*>(&S.a.zc[r * EW_ZP + 4 * lane]) = f32x4{};
  }
  if (g == 0) {
    if (lane < DAD_C) S.cnt[lane] = sel4i(cn, lane);
    if (ccand) { S.rowz[posc] = lane; S.wz[posc] = 1.0f; S.mem[posc] = 1; }
    if (ncand) { S.rowz[posn] = lane; S.wz[posn] = M.s; S.mem[posn] = 1; }
  }
  ECDA_CYC(16);
  {
    // the class of each row is wave-uniform: one add per row into its class's sum (a uniform
    // branch), not a select per class
    // branch-free: each row added to every class sum times a uniform 0/1 factor (adding
    // zeros leaves each sum bit-identical); a switch on the class made a branch per row and
    // register copies at every join (~2000 cycles)
    f32x4 cs0 = f32x4{}, cs1 = f32x4{}, cs2 = f32x4{}, cs3 = f32x4{};
#pragma unroll
    for (int u = 0; u < ECDA_PRE_U; ++u) {
      const int b = g + ECDA_NG * u;
      const int pk = __builtin_amdgcn_readfirstlane(b < Bn ? __builtin_amdgcn_readlane(prd, b < 64 ? b : 0) : -1);
      cs0 += ps[u] * (pk == 0 ? 1.0f : 0.0f);
      cs1 += ps[u] * (pk == 1 ? 1.0f : 0.0f);
      cs2 += ps[u] * (pk == 2 ? 1.0f : 0.0f);
      cs3 += ps[u] * (pk == 3 ? 1.0f : 0.0f);
    }
    *reinterpret_cast<f32x4*>(&S.c.cp[g][0][4 * lane]) = cs0;
    *reinterpret_cast<f32x4*>(&S.c.cp[g][1][4 * lane]) = cs1;
    *reinterpret_cast<f32x4*>(&S.c.cp[g][2][4 * lane]) = cs2;
    *reinterpret_cast<f32x4*>(&S.c.cp[g][3][4 * lane]) = cs3;
  }
  ECDA_CYC(17);
  // weight sum of the noisy members (I/utils.py:552-557), in every wave
  const double wsum_t = dad_wave_sum_d(ncand ? (double)M.s : 0.0);
  (void)cc;
  ECDA_CYC(18);
  ECDA_STAMP(2);
  __syncthreads();   // ---------------------------------------------------------------- 1
  ECDA_STAMP(3);
  if (wide)
    ecda_class_w<true>(a, c, S, M, ps, prd, ncls, nvalid, npairs, gc, rep_on, rep_coef, att_c, ncs, ncand_all, wsum_t);
  else
    ecda_class_w<false>(a, c, S, M, ps, prd, ncls, nvalid, npairs, gc, rep_on, rep_coef, att_c, ncs, ncand_all, wsum_t);
}

// block 0: the wave-centric tail; blocks 1..C: ECDA class blockIdx.x - 1.  Host contract:
// B <= 64, Bn <= 64, class-aware MMD (dad_tail_ecda otherwise).  Blocks > C pool the step's
// embeddings and logits first (pl.ready set; the tail and class blocks wait for them: pool_wait),
// which saves the separate dad_pool launch and its boundary.  Then (when pa.x16 is set):
// the NEXT step's row preparation (dad_prep.h) on the CUs the tail and the class blocks leave
// idle; it reads only the next batch and writes only the other prepared set, so it overlaps this
// step's latency-bound tail and ECDA.  The tail and class blocks have the lowest block ids, so
// they are dispatched first and never wait for a CU behind the preparation blocks.
// tail_w_s16.hip compiles this file again as dad_tail_ecda_w_s16: the same launch with the preparation
// reading rows of an fp16 / bf16 store (dad_prep_dispatch, S16).  A kernel and a unit of its own, so
// that this one holds the f32 preparation alone and compiles to what it did before the 16-bit stores.
// tail_w_rg.hip compiles it a third time as dad_tail_ecda_w_rg, the ragged step's launch: the pooling sums
// live slabs only and the preparation skips the rows of dead slabs (pool.h, dad_prep.h: RG), the rows read
// in the store's own type.
#if defined(DAD_TAIL_W_RG)
#define TAIL_W_KERNEL dad_tail_ecda_w_rg
#define DAD_TAIL_W_S16 1
#elif defined(DAD_TAIL_W_S16)
#define TAIL_W_KERNEL dad_tail_ecda_w_s16
#define DAD_TAIL_W_RG 0
#else
#define TAIL_W_KERNEL dad_tail_ecda_w
#define DAD_TAIL_W_S16 0
#define DAD_TAIL_W_RG 0
#endif
__global__ __launch_bounds__(TAIL_THREADS) void TAIL_W_KERNEL(DadTailArgs ta, DadEcdaArgs ca, DadPrepArgs pa,
                                                                DadPoolArgs pl) {
  DAD_GUARD_BLOCK(TAIL_THREADS);
  __shared__ union UW {
    TailW t;
    EcdaW e;
  } u;
  // fused pooling (pl.ready): the Bc + 2 Bn pool items (dad_pool's workgroups) on the spare
  // blocks' waves, item i on block i mod nx, wave i / nx (one item per CU first)
  const int nitems = pl.ready ? pl.g.Bc + 2 * pl.g.Bn : 0;
  if ((int)blockIdx.x > DAD_C) {
    constexpr int kWaves = TAIL_THREADS / 64;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int nx = (int)gridDim.x - 1 - DAD_C, xb = (int)blockIdx.x - 1 - DAD_C;
    for (int i = xb + nx * w; i < nitems; i += nx * kWaves) {
      pool_item<true, DAD_TAIL_W_RG>(pl, i, (int)threadIdx.x & 63);
      pool_publish(pl.ready, (int)threadIdx.x & 63);
    }
    if (!pa.x16) return;
#ifdef DAD_PROBE_STAMPS
    if ((threadIdx.x & 63) == 0 && xb < 256) prep_stamps[2 * (xb * kWaves + w)] = DAD_PROBE_WALL();
#endif
    dad_prep_dispatch<2, DAD_TAIL_W_S16, DAD_TAIL_W_RG>(pa, xb * kWaves + w, nx * kWaves, (int)threadIdx.x & 63);
#ifdef DAD_PROBE_STAMPS
    if (threadIdx.x == 0) atomicMax(&ecda_stamps[DAD_C * ECDA_SLOTS + 15], (unsigned long long)DAD_PROBE_WALL());
    if ((threadIdx.x & 63) == 0 && xb < 256) prep_stamps[2 * (xb * kWaves + w) + 1] = DAD_PROBE_WALL();
#endif
    return;
  }
  if (ta.cfg.B > TW_MAXB || ta.cfg.Bn > TW_MAXB) return;
  if (blockIdx.x == 0) TAIL_STAMP(14);   // launch entry (slot 15: the last preparation block's end)
  if (nitems) pool_wait(pl.ready, (uint32_t)nitems, pl.range_flag);
  if (blockIdx.x == 0) tail_block_w(ta, u.t);
  else ecda_block_w(ca, ta, (int)blockIdx.x - 1, u.e);
}
