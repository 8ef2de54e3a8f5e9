// The general "tail" of the DAD step: any batch up to DAD_MAX_BATCH per side, warm-up steps,
// the global-MMD ablation and DAD_TAIL_W=0 (batches of at most 64 per side otherwise take
// tail_w.hip's dad_tail_ecda_w).  Four launches:
//
//   dad_pool      (grid Bc + 2 Bn) : pooling finalisation + classifier forward (pool.h)
//   dad_tail      (1 block)        : CE(label smoothing), softmax, certainty, DACP thresholds and
//                                    mask, masked KL, classifier backward down to dL/dz
//                                                          I/train.py:397-471, I/utils.py:400-507
//                                    alone: warm-up steps
//   dad_ecda      (grid C)         : ECDALoss forward + backward, one workgroup per class, mask
//                                    and scores read from the tail's outputs      I/utils.py:510-652
//                                    alone: the modular dad_ecda_loss (utils_abi.hip)
//   dad_tail_ecda (grid 1 + C)     : both in one launch; the class blocks re-derive the mask
//
// The per-row arithmetic and the thresholds are tail_common.h's, shared with the wave-centric
// path; here rows are strided over the 512 threads of a block and partial sums are combined by
// fixed-order block reductions.
#include <type_traits>

#include "pool.h"
#include "tail_common.h"

__global__ __launch_bounds__(DAD_POOL_THREADS) void dad_pool(DadPoolArgs a) {
  DAD_GUARD_BLOCK(DAD_POOL_THREADS);
  pool_item<false>(a, (int)blockIdx.x, (int)threadIdx.x);
}
// the ragged step's pooling: live slabs only (pool.h, RG)
__global__ __launch_bounds__(DAD_POOL_THREADS) void dad_pool_rg(DadPoolArgs a) {
  DAD_GUARD_BLOCK(DAD_POOL_THREADS);
  pool_item<false, true>(a, (int)blockIdx.x, (int)threadIdx.x);
}

// ------------------------------------------------------------------------------ tail
// Latency design (one workgroup, ~30 dependent phases): every global input is requested at
// kernel entry -- logits, labels, the DACP state, W2 and the embedding values of the
// classifier backward -- so a single memory round trip is paid; the O(B^2) DACP ranks, the
// per-class epoch statistics and the b2 reduction are spread over the whole block with
// fixed-order (deterministic) combines instead of serial loops.
__device__ __forceinline__ void tail_block(const DadTailArgs& a, TailSmem& T) {
  const dad_config& cfg = a.cfg;
  const int B = cfg.B;                       // clean utterances
  const int Bn = cfg.warmup ? 0 : cfg.Bn;    // noisy utterances
  const int tid = threadIdx.x;
  double* dred = T.dred;
  auto& dred4 = T.dred4;
  float* fred = T.fred;
  auto& gz = T.gz;
  auto& sq = T.sq;
  float* ss = T.ss;
  int* sp = T.sp;
  float* sm = T.sm;
  float* dstate = T.dstate;
  float wc_unused[DAD_C];

  float* tf = a.tailf;
  float* extras = a.grad + DAD_NPARAM;
  const float* z0 = a.logits;
  const float* z1 = a.logits + (size_t)B * DAD_C;
  const float* z2 = a.logits + (size_t)(B + Bn) * DAD_C;
  const float eps = cfg.ls_eps;

  // ---- every global input up front (one round trip; consumed in this order)
  f32x4 zc = f32x4{}, zt = f32x4{}, zs = f32x4{};
  int yb = 0;
  if (tid < B) { zc = reinterpret_cast<const f32x4*>(z0)[tid]; yb = (int)a.yc[tid]; }
  if (tid < Bn) { zt = reinterpret_cast<const f32x4*>(z1)[tid]; zs = reinterpret_cast<const f32x4*>(z2)[tid]; }
  if (tid >= TAIL_THREADS - 20) dstate[tid - (TAIL_THREADS - 20)] = a.dacp[tid - (TAIL_THREADS - 20)];

  // ---- supervised CE with label smoothing on the clean logits (I/train.py:364,400)
  double ce_part = 0.0;
  for (int b = tid; b < B; b += TAIL_THREADS) {
    float z[4], lse, g[4];
    if (b == tid) { z[0] = zc[0]; z[1] = zc[1]; z[2] = zc[2]; z[3] = zc[3]; }
    else for (int c = 0; c < 4; ++c) z[c] = z0[b * 4 + c];
    const int y = b == tid ? yb : (int)a.yc[b];
    double loss;
    ce_row(z, y, eps, B, lse, g, loss);
#pragma unroll
    for (int c = 0; c < 4; ++c) gz[0][b][c] = g[c];
    ce_part += loss;
  }
  const double ce = block_sum_d(ce_part, dred) / (double)B;

  float kl = 0.0f, msum = 0.0f;
  int kl_on = 0;
  if (!cfg.warmup) {
    // ---- teacher probs (I/train.py:409-410) and certainty (I/utils.py:400-428)
    for (int b = tid; b < Bn; b += TAIL_THREADS) {
      float z[4], q[4], s;
      int pred;
      if (b == tid) { z[0] = zt[0]; z[1] = zt[1]; z[2] = zt[2]; z[3] = zt[3]; }
      else for (int c = 0; c < 4; ++c) z[c] = z1[b * 4 + c];
      teacher_certainty(z, cfg, q, s, pred);
      for (int c = 0; c < 4; ++c) sq[b][c] = q[c];
      ss[b] = s;
      sp[b] = pred;
    }
    if (tid < DAD_C) T.ncls[tid] = 0;
    __syncthreads();
    if (cfg.use_dacp) {
      // ---- DACPManager.calculate_mask (I/utils.py:449-507)
      dacp_thresholds(cfg, Bn, ss, sp, T.srt, T.ncls, dstate, T.tau_new, wc_unused, tf, extras);
      // mask, and the epoch statistics for update_class_quality_scores_epoch
      // (I/utils.py:503-505): per-class score sums and counts, fixed-order block reduction
      for (int b = tid; b < Bn; b += TAIL_THREADS) sm[b] = ss[b] >= T.tau_new[sp[b]] ? 1.0f : 0.0f;
      double st4[4] = {0.0, 0.0, 0.0, 0.0}, ct4[4] = {0.0, 0.0, 0.0, 0.0};
      for (int b = tid; b < Bn; b += TAIL_THREADS)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          st4[c] += sp[b] == c ? (double)ss[b] : 0.0;
          ct4[c] += sp[b] == c ? 1.0 : 0.0;
        }
      block_sum4_d(st4, dred4);
      block_sum4_d(ct4, dred4);
      if (tid < DAD_C) {
        extras[4 + tid] = (float)st4[tid];
        extras[8 + tid] = (float)ct4[tid];
      }
    } else {
      // fixed threshold (I/train.py:417-420): mask = float(max prob >= thr), weights = ones
      for (int b = tid; b < Bn; b += TAIL_THREADS) sm[b] = ss[b] >= cfg.fixed_thr ? 1.0f : 0.0f;
      if (tid < DAD_C) {
        tf[DAD_T_W + tid] = 1.0f;
        extras[0 + tid] = 0.0f;
        extras[4 + tid] = 0.0f;
        extras[8 + tid] = 0.0f;
      }
    }
    __syncthreads();
  }
  if (!cfg.warmup) {
    float mpart = 0.0f;
    for (int b = tid; b < Bn; b += TAIL_THREADS) mpart += sm[b];
    msum = block_sum_f(mpart, fred);
    kl_on = msum > 1.0f;   // I/train.py:444 (mask.sum().item() > 1)
    // ---- masked consistency KL(q || p_student) (I/train.py:445-447) + its logit grad
    double kl_part = 0.0;
    const float denom = msum + 1e-8f;
    for (int b = tid; b < Bn; b += TAIL_THREADS) {
      float z[4], klb, g[4];
      if (b == tid) { z[0] = zs[0]; z[1] = zs[1]; z[2] = zs[2]; z[3] = zs[3]; }
      else for (int c = 0; c < 4; ++c) z[c] = z2[b * 4 + c];
      const float q[4] = {sq[b][0], sq[b][1], sq[b][2], sq[b][3]};
      kl_row(z, q, sm[b], kl_on != 0, cfg.w_kl, denom, klb, g);
#pragma unroll
      for (int c = 0; c < 4; ++c) gz[1][b][c] = g[c];
      kl_part += (double)(klb * sm[b]);
    }
    const double kls = block_sum_d(kl_part, dred);
    kl = kl_on ? (float)(kls / (double)denom) : 0.0f;
  }
  // ---- per-sample outputs (noisy batch) for inspection / ECDA
  for (int b = tid; b < Bn; b += TAIL_THREADS) {
    tf[DAD_TAIL_HDR + b] = ss[b];
    tf[DAD_TAIL_HDR + Bn + b] = (float)sp[b];
    tf[DAD_TAIL_HDR + 2 * Bn + b] = sm[b];
    for (int c = 0; c < 4; ++c) tf[DAD_TAIL_HDR + 3 * Bn + b * 4 + c] = sq[b][c];
  }
  if (tid == 0) {
    tf[DAD_T_CE] = (float)ce;
    tf[DAD_T_KL] = kl;
    tf[DAD_T_SCL] = 0.0f;
    tf[DAD_T_MSUM] = msum;
    tf[DAD_T_KL_ON] = (float)kl_on;
    tf[DAD_T_ECDA_ON] = (kl_on && cfg.ecda_on) ? 1.0f : 0.0f;
  }
  __syncthreads();
  // ---- dL/dz of every utterance for the weight-gradient kernels (which rebuild the
  // classifier part of dL/de on the fly, I/model.py:62-63), the b2 grad, ECDA row flags
  for (int b = tid; b < B; b += TAIL_THREADS)
    *reinterpret_cast<f32x4*>(a.gzb + (size_t)b * DAD_C) = f32x4{gz[0][b][0], gz[0][b][1], gz[0][b][2], gz[0][b][3]};
  for (int b = tid; b < Bn; b += TAIL_THREADS)
    *reinterpret_cast<f32x4*>(a.gzb + (size_t)(B + b) * DAD_C) =
        f32x4{gz[1][b][0], gz[1][b][1], gz[1][b][2], gz[1][b][3]};
  double b2s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = tid; b < B; b += TAIL_THREADS)
#pragma unroll
    for (int c = 0; c < 4; ++c) b2s[c] += (double)gz[0][b][c];
  for (int b = tid; b < Bn; b += TAIL_THREADS)
#pragma unroll
    for (int c = 0; c < 4; ++c) b2s[c] += (double)gz[1][b][c];
  block_sum4_d(b2s, dred4);
  // (a select chain: indexed by tid the array went to scratch here, and to LDS in dad_tail_ecda)
  if (tid < 4) a.grad[DAD_OFF_B2 + tid] = (float)sel4d(b2s, tid);
}

__global__ __launch_bounds__(TAIL_THREADS) void dad_tail(DadTailArgs a) {
  DAD_GUARD_BLOCK(TAIL_THREADS);
  __shared__ TailSmem T;
  tail_block(a, T);
}

// ------------------------------------------------------------------------------ ECDA
// One workgroup per class (I/utils.py:601-632 loop body); the global-MMD ablation
// (I/utils.py:633-650) runs in workgroup 0.  Each workgroup only writes the embedding
// grads of ITS class members (clean: label == c, noisy: masked & pseudo-label == c), so
// no atomics are needed and the result is deterministic.
#define ECDA_NZ 80                          // members staged in LDS (n <= 80); larger sets read global
#define ECDA_PRE (ECDA_NG * ECDA_PRE_U)     // batches of at most this many rows prefetch every row

struct EcdaSmem {
  float z[ECDA_NZ * DAD_H];       // staged member embeddings (before that: centroid partials)
  float dm[ECDA_NZ * ECDA_NZ];    // pairwise distances, then symmetric MMD coefficients
  int idx[2 * DAD_MAX_BATCH];     // member list: [0,ns) clean rows, [ns,n) noisy rows
  float wt[2 * DAD_MAX_BATCH];    // member weights
  int pos[2 * ECDA_PRE];          // inverse of idx (prefetch path): clean row b -> [b], noisy row b -> [ECDA_PRE + b]
  float cent[DAD_C][DAD_H];
  double dred[ECDA_THREADS / 64][3];
  float fred[ECDA_THREADS / 64];
  int cnt_clean[DAD_C], cnt_noisy[DAD_C];
  int lab[DAD_MAX_BATCH];         // clean labels
  int prd[DAD_MAX_BATCH];         // noisy pseudo-labels, -1 where not masked in
  float scr[DAD_MAX_BATCH];       // noisy certainty scores
  int wcount[ECDA_THREADS / 64];
  float repg[DAD_H];              // repulsion grad of this class's noisy members, per hidden unit
};

// fixed-order block reduction of NV doubles (one barrier pair for all), valid in all threads
template <int NV>
__device__ __forceinline__ void ecda_block_sum_d(EcdaSmem& S, double (&v)[NV]) {
  static_assert(NV <= 3, "dred holds 3 values per wave");
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = dad_wave_sum_d(v[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) S.dred[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < ECDA_THREADS / 64; ++w) s += S.dred[w][k];
    v[k] = s;
  }
}

__device__ __forceinline__ float ecda_block_sum_f(EcdaSmem& S, float v) {
  v = dad_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) S.fred[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < ECDA_THREADS / 64; ++k) s += S.fred[k];
  return s;
}

// Ordered block-wide compaction: appends every i in [0, n) with flag(i) to S.idx (and
// weight(i) to S.wt) after position `base`, in ascending i; inv (nullable) gets i's position.
// Returns the new length.
template <typename Flag, typename Wgt>
__device__ int ecda_compact(EcdaSmem& S, int n, int base, Flag flag, Wgt weight, int* inv) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int c0 = 0; c0 < n; c0 += ECDA_THREADS) {
    const int i = c0 + tid;
    const bool f = i < n && flag(i);
    const float wi = f ? weight(i) : 0.0f;   // in flight across the barrier
    const uint64_t bal = __ballot(f);
    if (lane == 0) S.wcount[w] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < ECDA_THREADS / 64; ++k) {
      const int ck = S.wcount[k];
      pre += k < w ? ck : 0;
      tot += ck;
    }
    if (f) {
      const int pos = base + pre + __popcll(bal & ((1ull << lane) - 1ull));
      S.idx[pos] = i;
      S.wt[pos] = wi;
      if (inv) inv[i] = pos;
    }
    base += tot;
    __syncthreads();
  }
  return base;
}

// Member embeddings: staged in LDS when n <= ECDA_NZ, read from global otherwise.  The two
// cases are separate instantiations so that every access has a known address space (a
// run-time LDS-or-global select compiles to flat loads with full waits).
template <bool STAGED>
struct EcdaRows {
  const float* emb_c;
  const float* emb_s;
  EcdaSmem& S;
  int ns;
  __device__ __forceinline__ const float* row(int a) const {
    if constexpr (STAGED) return &S.z[a * DAD_H];
    else return (a < ns ? emb_c : emb_s) + (size_t)S.idx[a] * DAD_H;
  }
};

// staging from global rows (no prefetch: batches above ECDA_PRE rows)
__device__ __forceinline__ void ecda_stage_global(EcdaSmem& S, const float* emb_c, const float* emb_s, int ns, int n) {
#pragma unroll 4
  for (int k = threadIdx.x; k < n * (DAD_H / 4); k += ECDA_THREADS) {
    const int a = k / (DAD_H / 4), q = k - a * (DAD_H / 4);
    const float* src = (a < ns ? emb_c : emb_s) + (size_t)S.idx[a] * DAD_H;
    reinterpret_cast<f32x4*>(S.z)[k] = reinterpret_cast<const f32x4*>(src)[q];
  }
  __syncthreads();
}

// upper-triangle index t of an m x m matrix (row-major, diagonal included) -> (i, j), i <= j
__device__ __forceinline__ void ecda_tri(int t, int m, int& i, int& j) {
  const float b = 2.0f * (float)m + 1.0f;
  int r = (int)((b - sqrtf(fmaxf(b * b - 8.0f * (float)t, 0.0f))) * 0.5f);
  r = r < 0 ? 0 : (r >= m ? m - 1 : r);
  while (r > 0 && r * m - r * (r - 1) / 2 > t) --r;               // float rounding fix-ups
  while (r + 1 < m && (r + 1) * m - (r + 1) * r / 2 <= t) ++r;
  i = r;
  j = t - (r * m - r * (r - 1) / 2) + r;
}

// recursive-halving reduce-scatter of 16 per-lane values over KS adjacent slice lanes (KS <= 16):
// afterwards lane sl holds in v[0 .. 16/KS) the slice sums of values [base, base + 16/KS),
// base returned.  Every value is summed by the same tree over the slices (up to operand order
// of each add, which is commutative), so equal inputs give bit-equal sums in any lane.
template <int O, int M>
__device__ __forceinline__ void ecda_rs_level(float (&v)[16], int sl, int& base) {
  if constexpr (O > 0) {
    constexpr int HALF = M / 2;
    const bool up = (sl & O) != 0;
#pragma unroll
    for (int t = 0; t < HALF; ++t) {
      const float send = up ? v[t] : v[HALF + t];
      const float keep = up ? v[HALF + t] : v[t];
      v[t] = keep + __shfl_xor(send, O, 64);
    }
    base += up ? HALF : 0;
    ecda_rs_level<O / 2, HALF>(v, sl, base);
  }
}
template <int KS>
__device__ __forceinline__ int ecda_reduce_scatter(float (&v)[16], int sl) {
  int base = 0;
  ecda_rs_level<KS / 2, 16>(v, sl, base);
  return base;
}

// mmd = t_ss + t_tt - 2 t_st of _gaussian_kernel (I/utils.py:521-563) over members
// [0, ns) (clean embeddings) and [ns, n) (strong embeddings).  Leaves the symmetric
// coefficient matrix Csym = dmmd/dD + (dmmd/dD)^T in D, so that
// dmmd/dz_i = 2 sum_j Csym_ij (z_i - z_j).  Returns mmd (valid in all threads).
template <class RW>
__device__ __forceinline__ float ecda_mmd_coef(EcdaSmem& S, const RW& R, int n, float* D) {
  const int tid = threadIdx.x;
  const int ns = R.ns;
  // pairwise squared distances (I/utils.py:533-537), register-tiled over the upper triangle:
  // a work item is a 4x4 block (bi <= bj) of member pairs over one slice of the 256 hidden
  // units.  Per float4 step a lane loads 8 rows' values and does 16 pairs' differences.  The
  // slices per block (ks, a power of two) are chosen for the least per-SIMD time given the
  // round-robin wave placement; the slice lanes of a block are adjacent and combined by a
  // fixed butterfly.  Each block writes D[i][j] and D[j][i] from one value, and a diagonal
  // block computes (p, r) and (r, p) from exactly negated differences, so D is symmetric.
  const int nb = (n + 3) >> 2, nblk = nb * (nb + 1) / 2;
  // slices per block: least per-SIMD time, in units of 1/32 float4 step (a step: 8 row loads
  // and 64 packed VALU ops per lane; a reduce-scatter shuffle ~1/32 of that; 1/2 step setup)
  int lks = 0, best = 1 << 30;
  for (int l = 0; l <= 4; ++l) {
    const int waves = ((nblk << l) + 63) >> 6;
    const int cost = ((waves + 3) >> 2) * (((DAD_H / 4) >> l) * 32 + (16 - (16 >> l)) + 16);
    if (cost < best) { best = cost; lks = l; }
  }
  const int ks = 1 << lks, qs = (DAD_H / 4) >> lks;   // slices per block, float4 steps per slice
  const int nitem = nblk << lks;
  double part = 0.0;
  for (int it0 = 0; it0 < nitem; it0 += ECDA_THREADS) {   // uniform trip count: every lane shuffles
    const int item = it0 + tid;
    const bool on = item < nitem;
    const int sl = item & (ks - 1);
    int bi = 0, bj = 0;
    if (on) ecda_tri(item >> lks, nb, bi, bj);
    // packed accumulators: (sum over even dims, sum over odd dims) of each pair, so the
    // squares accumulate by v_pk_fma_f32 (half the VALU issues of scalar FMAs)
    f32x2 acc2[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc2[p][q] = f32x2{0.0f, 0.0f};
    if (on) {
      const f32x4* zi[4];
      const f32x4* zj[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        zi[p] = reinterpret_cast<const f32x4*>(R.row(min(4 * bi + p, n - 1))) + sl * qs;
        zj[p] = reinterpret_cast<const f32x4*>(R.row(min(4 * bj + p, n - 1))) + sl * qs;
      }
      const int rot = bi + bj + sl;   // spreads the lanes of a wave over the banks
      for (int q = 0; q < qs; ++q) {
        const int qq = (q + rot) & (qs - 1);
        f32x4 xi[4], xj[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          xi[p] = zi[p][qq];
          xj[p] = zj[p][qq];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 df = xi[p] - xj[r];
            const f32x2 lo = f32x2{df[0], df[1]}, hi = f32x2{df[2], df[3]};
            acc2[p][r] = __builtin_elementwise_fma(lo, lo, acc2[p][r]);
            acc2[p][r] = __builtin_elementwise_fma(hi, hi, acc2[p][r]);
          }
      }
    }
    float v[16];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * p + r] = acc2[p][r][0] + acc2[p][r][1];
    // combine the slices: lane sl ends with pairs [base, base + 16/ks) of the block
    int base = 0;
    switch (lks) {
      case 0: break;
      case 1: base = ecda_reduce_scatter<2>(v, sl); break;
      case 2: base = ecda_reduce_scatter<4>(v, sl); break;
      case 3: base = ecda_reduce_scatter<8>(v, sl); break;
      default: base = ecda_reduce_scatter<16>(v, sl); break;
    }
    if (on) {
      const int m = 16 >> lks;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        if (t >= m) break;
        const int k = base + t, p = k >> 2, r = k & 3;
        const int i = 4 * bi + p, j = 4 * bj + r;
        if (i < n && j < n && (bi < bj || p <= r)) {
          const float d = i == j ? 0.0f : v[t];
          D[i * n + j] = d;
          D[j * n + i] = d;
          part += i == j ? 0.0 : 2.0 * (double)d;
        }
      }
    }
  }
  double sd[1] = {part};
  ecda_block_sum_d<1>(S, sd);
  // detached bandwidth (I/utils.py:540-544): sum(D)/(n^2-n) / mul^(num//2), x mul^i
  float bw = (n > 1) ? (float)(sd[0] / (double)(n * n - n)) : 1.0f;
  bw = bw / 4.0f;
  float ibw[5];   // reciprocals: one division per bandwidth instead of ten per pair
#pragma unroll
  for (int m = 0; m < 5; ++m) ibw[m] = 1.0f / (bw * (float)(1 << m) + 1e-8f);
  // weight normalisers (I/utils.py:552-557)
  double wsum_t = 0.0;
  {
    int a = ns;
    for (; a + 8 <= n; a += 8) {   // eight weights per LDS round trip, summed in index order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = S.wt[a + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) wsum_t += v[u];
    }
    for (; a < n; ++a) wsum_t += S.wt[a];
  }
  const float Wss = (float)ns * (float)ns + 1e-8f;
  const float Wtt = (float)(wsum_t * wsum_t) + 1e-8f;
  const float Wst = (float)((double)ns * wsum_t) + 1e-8f;
  // terms and the symmetric coefficients Csym_ij = C_ij + C_ji, C = dmmd/dK * dK/dD, one
  // unordered pair per work item (K and dK computed once for (i, j) and (j, i))
  double t3[3] = {0.0, 0.0, 0.0};   // t_ss, t_tt, t_st numerators
  const int npair = n * (n + 1) / 2;
  for (int t = tid; t < npair; t += ECDA_THREADS) {
    int i, j;
    ecda_tri(t, n, i, j);
    const float d = D[i * n + j];
    float K = 0.0f, dK = 0.0f;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const float e = __expf(-d * ibw[m]);
      K += e;
      dK -= e * ibw[m];
    }
    const double mult = i == j ? 1.0 : 2.0;   // (i, j) and (j, i) of the sums
    float cs;
    if (j < ns) {                               // both clean
      t3[0] += mult * (double)K;
      cs = (i == j ? 1.0f : 2.0f) / Wss;
    } else if (i >= ns) {                       // both noisy
      const float ww = S.wt[i] * S.wt[j];
      t3[1] += mult * ((double)K * ww);
      cs = (i == j ? 1.0f : 2.0f) * ww / Wtt;
    } else {                                    // (i, j) in S x T; (j, i) in T x S is unused by t_st
      t3[2] += (double)K * S.wt[j];
      cs = -2.0f * S.wt[j] / Wst;
    }
    const float v = cs * dK;
    D[i * n + j] = v;
    D[j * n + i] = v;
  }
  ecda_block_sum_d<3>(S, t3);   // its barriers also publish D
  const float mmd = (float)(t3[0] / Wss + t3[1] / Wtt - 2.0 * (t3[2] / Wst));
  return mmd;
}

// Embedding grads of the members into the ECDA part of dL/de (plain stores; a row belongs to
// at most one class), register-tiled: a work item is 4 members x 4 hidden units (one float4
// column chunk), so each member row chunk read from LDS serves 4 members' sums:
//   g = mmd_scale * 2 sum_j Csym_ij (z_i - z_j)            (all members, if D)
//     + comp_scale * (z_i - mu_c) + repg                     (noisy members)
// comp_part accumulates sum ||z_i - mu_c||^2 over noisy members (when cent).
template <class RW>
__device__ __forceinline__ void ecda_member_grads(EcdaSmem& S, const RW& R, int n, const float* D,
                                                  float mmd_scale, const float* cent, float comp_scale,
                                                  const float* repg, float* ge_c, float* ge_s, uint32_t* eflag,
                                                  int B_, float& comp_part) {
  const int ns = R.ns;
  const int nb = (n + 3) >> 2;
  for (int item = threadIdx.x; item < nb * (DAD_H / 4); item += ECDA_THREADS) {
    const int ib = item / (DAD_H / 4), hq = item - ib * (DAD_H / 4);
    int m[4];
    f32x4 zi[4], acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      m[p] = min(4 * ib + p, n - 1);
      zi[p] = reinterpret_cast<const f32x4*>(R.row(m[p]))[hq];
      acc[p] = f32x4{};
    }
    if (D) {
      // four members j per round: every LDS read of the round issued before its FMAs
      int j = 0;
      for (; j + 4 <= n; j += 4) {
        f32x4 zj[4];
        float cj[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          zj[u] = reinterpret_cast<const f32x4*>(R.row(j + u))[hq];
#pragma unroll
          for (int p = 0; p < 4; ++p) cj[u][p] = D[(j + u) * n + m[p]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int p = 0; p < 4; ++p)   // Csym[j][i] = Csym[i][j]; packed sub + packed FMA
            acc[p] = __builtin_elementwise_fma(f32x4{cj[u][p], cj[u][p], cj[u][p], cj[u][p]}, zi[p] - zj[u], acc[p]);
      }
      for (; j < n; ++j) {
        const f32x4 zj = reinterpret_cast<const f32x4*>(R.row(j))[hq];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float cji = D[j * n + m[p]];
          acc[p] = __builtin_elementwise_fma(f32x4{cji, cji, cji, cji}, zi[p] - zj, acc[p]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int mm = 4 * ib + p;
      if (mm >= n) break;
      f32x4 g = D ? mmd_scale * (2.0f * acc[p]) : f32x4{};
      if (mm >= ns) {
        if (cent) {
          const f32x4 df = zi[p] - reinterpret_cast<const f32x4*>(cent)[hq];
          comp_part += ((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]) + df[3] * df[3];
          g += comp_scale * df;
        }
        g += reinterpret_cast<const f32x4*>(repg)[hq];
      }
      reinterpret_cast<f32x4*>((mm < ns ? ge_c : ge_s) + (size_t)S.idx[mm] * DAD_H)[hq] = g;
      if (hq == 0) eflag[mm < ns ? S.idx[mm] : B_ + S.idx[mm]] = 1u;
    }
  }
}

// DACP state and thresholds of the fused prefix (dad_tail_ecda's ECDA blocks)
struct EcdaPrefix {
  float dstate[20];
  int ncls[DAD_C];
  float tau_new[DAD_C];
  float wc[DAD_C];
  float fred[16];
};

// One class of ECDA.  FUSED: the DACP mask, scores and class weights are derived here from
// the teacher logits by the same code as the tail block (teacher_certainty, dacp_thresholds),
// instead of being read back from the tail's outputs.
// Batches of at most ECDA_PRE rows per side load every embedding row into registers at entry
// (wave g holds rows g, g + 8, ... of column chunk lane), in flight during the metadata phase;
// the centroid pass and the member staging then need no global round trip.
template <bool FUSED>
__device__ __forceinline__ void ecda_block(const DadEcdaArgs& a, const int c, EcdaSmem& S, float (&pdist)[DAD_C][DAD_C],
                                           const DadTailArgs* ta, EcdaPrefix& P) {
  const dad_config& cfg = a.cfg;
  const int B = cfg.B, Bn = cfg.Bn;
  const int tid = threadIdx.x;
  const int g = tid >> 6, lq = tid & 63;
  const float* tf = a.tailf;
  const float* emb_c = a.emb;
  const float* emb_s = a.emb + (size_t)(B + Bn) * DAD_H;
  float* ge_c = a.ge;
  float* ge_s = a.ge + (size_t)B * DAD_H;
  float* scratch = a.scratch + (size_t)c * (B + Bn) * (B + Bn);
  const float wscale = cfg.w_ecda;
  float ecda_on;
  const float* w;   // DACP class weights
  const bool pre = B <= ECDA_PRE && Bn <= ECDA_PRE;
  f32x4 pc[ECDA_PRE_U], ps[ECDA_PRE_U];
  if (FUSED) {
    // teacher logits first: the DACP prefix waits on them
    f32x4 zt = f32x4{};
    const float* z1 = ta->logits + (size_t)B * DAD_C;
    if (tid < Bn) zt = reinterpret_cast<const f32x4*>(z1)[tid];
    if (tid >= ECDA_THREADS - 20) P.dstate[tid - (ECDA_THREADS - 20)] = ta->dacp[tid - (ECDA_THREADS - 20)];
    for (int b = tid; b < B; b += ECDA_THREADS) S.lab[b] = (int)a.yc[b];
    if (pre) {
#pragma unroll
      for (int u = 0; u < ECDA_PRE_U; ++u) {
        const int b = g + ECDA_NG * u;
        pc[u] = b < B ? reinterpret_cast<const f32x4*>(emb_c + (size_t)b * DAD_H)[lq] : f32x4{};
        ps[u] = b < Bn ? reinterpret_cast<const f32x4*>(emb_s + (size_t)b * DAD_H)[lq] : f32x4{};
      }
    }
    for (int b = tid; b < Bn; b += ECDA_THREADS) {
      float z[4], q[4], sc;
      int pred;
      if (b == tid) { z[0] = zt[0]; z[1] = zt[1]; z[2] = zt[2]; z[3] = zt[3]; }
      else for (int k = 0; k < 4; ++k) z[k] = z1[b * 4 + k];
      teacher_certainty(z, cfg, q, sc, pred);
      S.scr[b] = sc;
      S.prd[b] = pred;
    }
    if (tid < DAD_C) { P.ncls[tid] = 0; S.cnt_clean[tid] = 0; S.cnt_noisy[tid] = 0; }
    __syncthreads();
    // masked-out noisy samples get pseudo-label -1 (noisy_mask>thr re-cast: I/utils.py:573-576)
    if (cfg.use_dacp) {
      dacp_thresholds(cfg, Bn, S.scr, S.prd, reinterpret_cast<float(*)[DAD_MAX_BATCH]>(S.z), P.ncls, P.dstate,
                      P.tau_new, P.wc, nullptr, nullptr);
      for (int b = tid; b < Bn; b += ECDA_THREADS) S.prd[b] = S.scr[b] >= P.tau_new[S.prd[b]] ? S.prd[b] : -1;
    } else {
      for (int b = tid; b < Bn; b += ECDA_THREADS) S.prd[b] = S.scr[b] >= cfg.fixed_thr ? S.prd[b] : -1;
      if (tid < DAD_C) P.wc[tid] = 1.0f;
    }
    float mpart = 0.0f;
    for (int b = tid; b < Bn; b += ECDA_THREADS) mpart += S.prd[b] >= 0 ? 1.0f : 0.0f;
    const float msum = block_sum_f(mpart, P.fred);   // the tail's mask sum (exact: a count)
    ecda_on = (msum > 1.0f && cfg.ecda_on) ? 1.0f : 0.0f;   // I/train.py:444
    w = P.wc;
  } else {
    ecda_on = tf[DAD_T_ECDA_ON];   // branched on after the metadata loads are issued
    w = tf + DAD_T_W;
    const float* score = tf + DAD_TAIL_HDR;
    const float* predf = tf + DAD_TAIL_HDR + Bn;
    const float* mask = tf + DAD_TAIL_HDR + 2 * Bn;
    // stage per-sample metadata (masked-out noisy samples get pseudo-label -1)
    for (int b = tid; b < B; b += ECDA_THREADS) S.lab[b] = (int)a.yc[b];
    for (int b = tid; b < Bn; b += ECDA_THREADS) {
      S.prd[b] = mask[b] > 0.0f ? (int)predf[b] : -1;   // noisy_mask>thr re-cast: I/utils.py:573-576
      S.scr[b] = score[b];
    }
    if (pre) {
#pragma unroll
      for (int u = 0; u < ECDA_PRE_U; ++u) {
        const int b = g + ECDA_NG * u;
        pc[u] = b < B ? reinterpret_cast<const f32x4*>(emb_c + (size_t)b * DAD_H)[lq] : f32x4{};
        ps[u] = b < Bn ? reinterpret_cast<const f32x4*>(emb_s + (size_t)b * DAD_H)[lq] : f32x4{};
      }
    }
    if (tid < DAD_C) { S.cnt_clean[tid] = 0; S.cnt_noisy[tid] = 0; }
  }
  __syncthreads();
  if (ecda_on == 0.0f) return;   // no row flagged: the ECDA part of dL/de is zero

  // member rows into S.z at their compacted positions: from the registers (prefetch), or
  // from global rows through S.idx
  auto stage = [&](int ns, int n) {
    if (pre) {
      // every position read before the first store (one LDS round trip); -1: not a member
      int pcl[ECDA_PRE_U], pno[ECDA_PRE_U];
#pragma unroll
      for (int u = 0; u < ECDA_PRE_U; ++u) {
        const int b = g + ECDA_NG * u;   // < ECDA_PRE: S.pos rows past B / Bn stay -1
        pcl[u] = S.pos[b];
        pno[u] = S.pos[ECDA_PRE + b];
      }
#pragma unroll
      for (int u = 0; u < ECDA_PRE_U; ++u) {
        if (pcl[u] >= 0) reinterpret_cast<f32x4*>(&S.z[pcl[u] * DAD_H])[lq] = pc[u];
        if (pno[u] >= 0) reinterpret_cast<f32x4*>(&S.z[pno[u] * DAD_H])[lq] = ps[u];
      }
      __syncthreads();
    } else {
      ecda_stage_global(S, emb_c, emb_s, ns, n);
    }
  };
  int* inv = pre ? S.pos : nullptr;

  if (!cfg.class_aware) {
    // global MMD ablation: all clean vs all masked noisy, unit weights (I/utils.py:633-650)
    if (c != 0) return;
    if (tid < DAD_H) S.repg[tid] = 0.0f;   // no repulsion term (read after the compaction's barriers)
    if (pre && tid < 2 * ECDA_PRE) S.pos[tid] = -1;
    int n = ecda_compact(S, B, 0, [](int) { return true; }, [](int) { return 1.0f; }, inv);
    const int ns = n;
    n = ecda_compact(S, Bn, n, [&](int i) { return S.prd[i] >= 0; }, [](int) { return 1.0f; },
                     inv ? inv + ECDA_PRE : nullptr);
    const int nt = n - ns;
    if (ns >= 2 && nt >= 2) {
      auto run = [&](auto staged_tag) {
        constexpr bool ST = decltype(staged_tag)::value;
        const EcdaRows<ST> R{emb_c, emb_s, S, ns};
        float* D = ST ? S.dm : scratch;
        if constexpr (ST) stage(ns, n);
        const float mmd = ecda_mmd_coef(S, R, n, D);
        float unused = 0.0f;
        ecda_member_grads(S, R, n, D, wscale, nullptr, 0.0f, S.repg, ge_c, ge_s, a.eflag, B, unused);
        if (tid == 0) { a.tail_terms[0] = mmd; a.tail_terms[DAD_T_ECDA_GATE - DAD_T_ECDA_TERM] = 1.0f; }
      };
      if (n <= ECDA_NZ) run(std::true_type{});
      else run(std::false_type{});
    }
    return;
  }

  // class-aware path.  In fixed-threshold mode class_weights_wce = ones(Bn) (I/train.py:420)
  // so the loop runs over range(Bn): only classes < min(Bn, C) can have members.
  const int ncls = cfg.use_dacp ? DAD_C : (Bn < DAD_C ? Bn : DAD_C);
  if (c >= ncls) return;
  for (int b = tid; b < B; b += ECDA_THREADS)
    if (S.lab[b] >= 0 && S.lab[b] < ncls) atomicAdd(&S.cnt_clean[S.lab[b]], 1);
  for (int b = tid; b < Bn; b += ECDA_THREADS)
    if (S.prd[b] >= 0 && S.prd[b] < ncls) atomicAdd(&S.cnt_noisy[S.prd[b]], 1);
  if (pre && tid < 2 * ECDA_PRE) S.pos[tid] = -1;
  // noisy centroids of every class (needed for the repulsion term): row group g (one wave) x
  // 64 float4 columns, partials combined in fixed group order
  {
    float* part = S.z;   // [NG groups][C][H], before the members are staged
    static_assert(ECDA_NG * DAD_C * DAD_H <= ECDA_NZ * DAD_H, "centroid partials must fit in S.z");
    f32x4 cs[DAD_C];
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) cs[k] = f32x4{};
    if (pre) {
      int pk[ECDA_PRE_U];
#pragma unroll
      for (int u = 0; u < ECDA_PRE_U; ++u) {   // all pseudo-labels first (one LDS round trip)
        const int b = g + ECDA_NG * u;
        pk[u] = S.prd[b < Bn ? b : 0];
        pk[u] = b < Bn ? pk[u] : -1;
      }
#pragma unroll
      for (int u = 0; u < ECDA_PRE_U; ++u)
#pragma unroll
        for (int k = 0; k < DAD_C; ++k) cs[k] += pk[u] == k ? ps[u] : f32x4{};
    } else {
#pragma unroll 4
      for (int b = g; b < Bn; b += ECDA_NG) {
        const int pk = S.prd[b];
        const f32x4 e = reinterpret_cast<const f32x4*>(emb_s + (size_t)b * DAD_H)[lq];
#pragma unroll
        for (int k = 0; k < DAD_C; ++k) cs[k] += pk == k ? e : f32x4{};
      }
    }
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) reinterpret_cast<f32x4*>(part + (g * DAD_C + k) * DAD_H)[lq] = cs[k];
    __syncthreads();
    for (int e = tid; e < DAD_C * DAD_H; e += ECDA_THREADS) {
      const int k = e / DAD_H, hh = e & (DAD_H - 1);
      float sk = 0.0f;
#pragma unroll
      for (int gg = 0; gg < ECDA_NG; ++gg) sk += part[(gg * DAD_C + k) * DAD_H + hh];
      S.cent[k][hh] = S.cnt_noisy[k] > 0 ? sk / (float)S.cnt_noisy[k] : 0.0f;
    }
  }
  __syncthreads();
  // per-class counts into registers (one LDS round trip for all of them)
  int cn[DAD_C], cc[DAD_C];
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) { cn[k] = S.cnt_noisy[k]; cc[k] = S.cnt_clean[k]; }
  // class attention (I/utils.py:597-599)
  float att[DAD_C];
  if (cfg.use_dacp) {
    float wk[DAD_C];
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) wk[k] = w[k];
    const float wmean = (((wk[0] + wk[1]) + wk[2]) + wk[3]) / 4.0f;
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) att[k] = expf(cfg.ecda_att_lambda * (wmean - wk[k]));
  } else {
#pragma unroll
    for (int k = 0; k < DAD_C; ++k) att[k] = 1.0f;
  }
  const float att_c = att[c];
  // repulsion over valid centroids (I/utils.py:582-595)
  int nvalid = 0;
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) nvalid += (k < ncls && cn[k] > 0) ? 1 : 0;
  const int npairs = nvalid * (nvalid - 1) / 2;
  {
    // 16 (p, q) pairs x 256 dims over all threads: 32 threads per pair, 8 dims each,
    // combined by a 32-lane reduction (pair-symmetric order, so pdist stays symmetric)
    const int pair = tid / 32, l32 = tid & 31;
    float d = 0.0f;
    if (pair < DAD_C * DAD_C) {
      const int p = pair / DAD_C, q = pair % DAD_C;
      const int lo = p < q ? p : q, hi = p < q ? q : p;
      if (p < ncls && q < ncls && S.cnt_noisy[p] > 0 && S.cnt_noisy[q] > 0 && p != q) {
        const f32x4* a0 = reinterpret_cast<const f32x4*>(&S.cent[lo][l32 * (DAD_H / 32)]);
        const f32x4* a1 = reinterpret_cast<const f32x4*>(&S.cent[hi][l32 * (DAD_H / 32)]);
        const f32x4 x0 = a0[0], x1 = a0[1], y0 = a1[0], y1 = a1[1];
        const float v[8] = {x0[0] - y0[0], x0[1] - y0[1], x0[2] - y0[2], x0[3] - y0[3],
                            x1[0] - y1[0], x1[1] - y1[1], x1[2] - y1[2], x1[3] - y1[3]};
#pragma unroll
        for (int k = 0; k < 8; ++k) d += v[k] * v[k];
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) d += __shfl_xor(d, o, 32);
    if (pair < DAD_C * DAD_C && l32 == 0) pdist[pair / DAD_C][pair % DAD_C] = sqrtf(d);
  }
  __syncthreads();
  float pd[DAD_C][DAD_C];
#pragma unroll
  for (int p = 0; p < DAD_C; ++p)
#pragma unroll
    for (int q = 0; q < DAD_C; ++q) pd[p][q] = pdist[p][q];
  float rep = 0.0f;
  if (nvalid > 1) {
    float sp = 0.0f;
#pragma unroll
    for (int p = 0; p < DAD_C; ++p)
#pragma unroll
      for (int q = p + 1; q < DAD_C; ++q)
        if (q < ncls && cn[p] > 0 && cn[q] > 0) sp += pd[p][q];
    rep = -sp / (float)npairs;
  }
  bool gated[DAD_C];
  float rep_coef = 0.0f;
#pragma unroll
  for (int k = 0; k < DAD_C; ++k) {
    gated[k] = k < ncls && cc[k] >= 2 && cn[k] >= 2;   // I/utils.py:609-610
    if (gated[k]) rep_coef += att[k] * cfg.ecda_delta;
  }
  // repulsion grad of this class's noisy members (d rep / d mu_c, then 1/n_c per member)
  const bool rep_on = nvalid > 1 && cn[c] > 0 && rep_coef != 0.0f;
  if (tid < DAD_H) {
    const int hh = tid;
    float rep_g = 0.0f;
    if (rep_on) {
      float ce[DAD_C];
#pragma unroll
      for (int q = 0; q < DAD_C; ++q) ce[q] = S.cent[q][hh];
      float gsum = 0.0f;
#pragma unroll
      for (int q = 0; q < DAD_C; ++q) {
        if (q == c || q >= ncls || cn[q] == 0) continue;
        const float nd = pd[c][q];
        if (nd > 0.0f) gsum += (ce[c] - ce[q]) / nd;
      }
      rep_g = wscale * rep_coef * (-gsum / (float)npairs / (float)cn[c]);
    }
    S.repg[hh] = rep_g;   // read after the member compaction's barriers
  }
  if (!gated[c] && !rep_on) return;
  // members of class c: clean (label c, weight 1) then masked noisy (pseudo-label c, weight = score);
  // a class below the gate only needs its noisy members (repulsion)
  int n = gated[c] ? ecda_compact(S, B, 0, [&](int i) { return S.lab[i] == c; }, [](int) { return 1.0f; }, inv) : 0;
  const int ns = n;
  n = ecda_compact(S, Bn, n, [&](int i) { return S.prd[i] == c; }, [&](int i) { return S.scr[i]; },
                   inv ? inv + ECDA_PRE : nullptr);
  const int nt = n - ns;
  float mmd = 0.0f;
  float cpart = 0.0f;
  auto run = [&](auto R, float* Dbuf) {
    constexpr bool ST = std::is_same_v<decltype(R), EcdaRows<true>>;
    float* D = nullptr;
    if (gated[c]) {
      D = Dbuf;
      if constexpr (ST) stage(ns, n);
      mmd = ecda_mmd_coef(S, R, n, D);
    }   // (a repulsion-only class needs no member rows: g = repg)
    // compactness (I/utils.py:614-616): mean_j ||z_j - mu||^2, grad (2/nt)(z_j - mu)
    ecda_member_grads(S, R, n, D, wscale * att_c, gated[c] ? S.cent[c] : nullptr,
                      wscale * att_c * cfg.ecda_gamma * (2.0f / (float)nt), S.repg, ge_c, ge_s, a.eflag, B, cpart);
  };
  if (n <= ECDA_NZ) run(EcdaRows<true>{emb_c, emb_s, S, ns}, S.dm);
  else run(EcdaRows<false>{emb_c, emb_s, S, ns}, scratch);
  if (!gated[c]) return;
  const float comp = ecda_block_sum_f(S, cpart) / (float)nt;
  if (tid == 0) {
    a.tail_terms[c] = att_c * (mmd + cfg.ecda_gamma * comp + cfg.ecda_delta * rep);
    a.tail_terms[DAD_T_ECDA_GATE - DAD_T_ECDA_TERM + c] = 1.0f;
  }
}

__global__ __launch_bounds__(ECDA_THREADS) void dad_ecda(DadEcdaArgs a) {
  DAD_GUARD_BLOCK(ECDA_THREADS);
  __shared__ struct { EcdaSmem s; float pdist[DAD_C][DAD_C]; EcdaPrefix p; } u;
  ecda_block<false>(a, blockIdx.x, u.s, u.pdist, nullptr, u.p);
}

// block 0: the tail (losses, DACP outputs, dL/dz); blocks 1..C: ECDA class blockIdx.x - 1,
// which re-derives the DACP mask itself and so does not wait for block 0.  The two roles
// write disjoint outputs (dad_pool zeroed the ECDA flags and terms).  LDS: one union.
static_assert(DAD_TAIL_THREADS == DAD_ECDA_THREADS, "dad_tail_ecda: one block size for both roles");
__global__ __launch_bounds__(TAIL_THREADS) void dad_tail_ecda(DadTailArgs ta, DadEcdaArgs ca) {
  DAD_GUARD_BLOCK(TAIL_THREADS);
  __shared__ union U {
    TailSmem t;
    struct E { EcdaSmem s; float pdist[DAD_C][DAD_C]; EcdaPrefix p; } e;
  } u;
  if (blockIdx.x == 0) tail_block(ta, u.t);
  else {
    ecda_block<true>(ca, (int)blockIdx.x - 1, u.e.s, u.e.pdist, &ta, u.e.p);
  }
}
