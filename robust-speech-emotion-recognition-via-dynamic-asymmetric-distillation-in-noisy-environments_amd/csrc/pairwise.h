// The n x n pass over the fp32 Gram block of two 64-row tiles of centred embeddings, shared by the class-separation
// pass (cluster.hip) and the t-SNE affinities (tsne.hip): one definition of the operand layout, the column tile's
// staging, the MFMA chain, the walk of a row tile over its column tiles, the squared distance and the column-chunk
// plan, so both passes (and dad_cluster_norms, the diagonal of the same block) produce the same bits from the same
// rows.
//
//   A operand   row ia of the row tile, lane = row (l32), 4 consecutive k per k-block of 8 and lane half (kh):
//               MFMA step e of k-block q takes k = 8 q + 4 kh + e on both operands
//   B operand   the column tile's rows in LDS, row stride kGramLd = 260 floats (the 16-byte operand reads of 8
//               consecutive rows cover the 32 banks once)
//   result      acc[r] = (x_row - mu).(x_col - mu), row = dad_acc_row(r, kh) of the wave's 32 rows, col = l32
#ifndef DAD_PAIRWISE_H_
#define DAD_PAIRWISE_H_
#include "dad_common.h"

constexpr int kGramTile = 64;              // rows and columns of a tile
constexpr int kGramLd = DAD_H + 4;         // LDS row stride of the column tile, floats
constexpr int kGramThreads = 256;          // 4 waves: (row half, column half) quadrants of 32 x 32

// |x_i - mu|^2 per row as the diagonal of the Gram block (cluster.hip); norms has ceil(n / 64) * 64 entries, padding
// rows get 0.  Grid ceil(n / 64), 128 threads.
__global__ void dad_cluster_norms(const float* __restrict__ emb, const float* __restrict__ mean, int n,
                                  float* __restrict__ norms);

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// row ia's A operand (zeros for ia >= n, which is not read)
__device__ __forceinline__ void dad_gram_load_a(f32x4 (&av)[DAD_H / 8], const float* __restrict__ emb,
                                                const float* __restrict__ mean, int ia, int n, int kh) {
  const float* ra = emb + (size_t)(ia < n ? ia : 0) * DAD_H + 4 * kh;
#pragma unroll
  for (int q = 0; q < DAD_H / 8; ++q)
    av[q] = ia < n ? *reinterpret_cast<const f32x4*>(ra + 8 * q) - *reinterpret_cast<const f32x4*>(mean + 4 * kh + 8 * q)
                   : f32x4{};
}

// rows j0 .. j0 + 63 minus mu into bt (zeros for rows >= n, which are not read); mu4 = mean[4 (tid & 63) ..]
__device__ __forceinline__ void dad_gram_stage(float* __restrict__ bt, const float* __restrict__ emb, f32x4 mu4,
                                               int j0, int n, int tid) {
#pragma unroll
  for (int e = 0; e < kGramTile * (DAD_H / 4) / kGramThreads; ++e) {
    const int idx = tid + kGramThreads * e, r = idx >> 6, c4 = 4 * (idx & 63), j = j0 + r;   // (idx & 63 = tid & 63)
    const f32x4 v = j < n ? *reinterpret_cast<const f32x4*>(emb + (size_t)j * DAD_H + c4) - mu4 : f32x4{};
    *reinterpret_cast<f32x4*>(&bt[r * kGramLd + c4]) = v;
  }
}

// the chain of 128 MFMAs of the wave's rows against column jc of the staged tile
__device__ __forceinline__ f32x16 dad_gram_block(const f32x4 (&av)[DAD_H / 8], const float* __restrict__ bt, int jc,
                                                 int kh) {
  const float* rb = &bt[jc * kGramLd + 4 * kh];
  f32x16 acc = f32x16{};
#pragma unroll
  for (int q = 0; q < DAD_H / 8; ++q) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(rb + 8 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][e], bv[e], acc, 0, 0, 0);
  }
  return acc;
}

// The squared distance of global rows ig and jg from their norms and their Gram entry: max((|a_i|^2 + |a_j|^2) -
// 2 a_i.a_j, 0), and exactly 0 on the diagonal.  The only definition: dad_cluster_metrics takes its square root and
// dad_tsne_affinities stores it, which is what include/dad.h promises of the two (an exact duplicate row's norm and
// Gram entry are the same bits, so its distance is exactly 0 in both).
__device__ __forceinline__ float dad_pair_d2(float ni, float nj, float dot, int ig, int jg) {
  const float d2 = fmaxf((ni + nj) - 2.0f * dot, 0.0f);
  return ig == jg ? 0.0f : d2;
}

// A thread's place in the walk: wave (rh, ch) owns the 32 x 32 quadrant (row half, column half) of every tile
struct GramLane {
  int kh, l32, rh, ch;
};
__device__ __forceinline__ GramLane dad_gram_lane(int tid) {
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  return GramLane{(tid & 63) >> 5, tid & 31, w >> 1, w & 1};
}

// The walk of the workgroup's row tile (rows i0 .. i0 + 63) against the column tiles t0, t0 + step, ... < t1, by
// kGramThreads threads.  bt [64 * kGramLd], nj_s [64] and ni_s [64] are the caller's LDS.  Per column tile, between
// the two barriers, thread tid < 64 runs extra(tid, j) for its column j = 64 t + tid (what the caller stages besides
// the norms); behind them every thread runs epi(r, ig, jc, jg, d2) for its 16 entries: accumulator entry r, global row
// ig, column jc of the tile = global column jg, d2 = dad_pair_d2.  Rows and columns >= n take part with zero operands:
// the caller's epi leaves them out.  norms is read unguarded: it has 64 * ceil(n / 64) entries and dad_cluster_norms
// writes 0 to the padding.  The last tile's operand reads are not fenced: a caller that reuses bt puts a barrier first.
template <typename Extra, typename Epi>
__device__ __forceinline__ void dad_gram_walk(const float* __restrict__ emb, const float* __restrict__ norms,
                                              const float* __restrict__ mean, int n, int i0, int t0, int t1, int step,
                                              float* __restrict__ bt, float* __restrict__ nj_s, float* __restrict__ ni_s,
                                              Extra extra, Epi epi) {
  const int tid = threadIdx.x;
  const GramLane g = dad_gram_lane(tid);
  f32x4 av[DAD_H / 8];
  dad_gram_load_a(av, emb, mean, i0 + 32 * g.rh + g.l32, n, g.kh);
  const f32x4 mu4 = *reinterpret_cast<const f32x4*>(mean + 4 * (tid & 63));   // the columns this thread stages
  if (tid < kGramTile) ni_s[tid] = norms[i0 + tid];
  for (int t = t0; t < t1; t += step) {
    const int j0 = kGramTile * t;
    __syncthreads();      // the previous tile's operand reads are done
    dad_gram_stage(bt, emb, mu4, j0, n, tid);
    if (tid < kGramTile) {
      nj_s[tid] = norms[j0 + tid];
      extra(tid, j0 + tid);
    }
    __syncthreads();
    const int jc = 32 * g.ch + g.l32, jg = j0 + jc;
    const f32x16 acc = dad_gram_block(av, bt, jc, g.kh);
    const float nj = nj_s[jc];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = 32 * g.rh + dad_acc_row(r, g.kh), ig = i0 + il;
      epi(r, ig, jc, jg, dad_pair_d2(ni_s[il], nj, acc[r], ig, jg));
    }
  }
}

// The column chunks of a row tile: rt tiles in `chunks` contiguous runs of `per` (the last may be shorter), for `want`
// asked-for chunks clamped to [1, min(rt, max_chunks)]; no chunk is empty.
struct PairPlan {
  int rt, chunks, per;
};
inline PairPlan pair_plan(int64_t n, int want, int max_chunks) {
  PairPlan p;
  p.rt = (int)((n + kGramTile - 1) / kGramTile);
  const int cap = p.rt < max_chunks ? p.rt : max_chunks;
  want = want < 1 ? 1 : (want > cap ? cap : want);
  p.per = (p.rt + want - 1) / want;
  p.chunks = (p.rt + p.per - 1) / p.per;
  return p;
}

// the plan of `chunks` asked-for chunks, or for chunks <= 0 the planner's (dad_cluster_plan, dad_tsne_plan) for the
// current device
inline int pair_resolve(int64_t n, int chunks, int max_chunks, int (*planner)(int64_t, int, int*, int*, int*),
                        PairPlan* p) {
  if (chunks > 0) {
    *p = pair_plan(n, chunks, max_chunks);
    return DAD_OK;
  }
  int cus = 0;
  DAD_RET(device_cus(&cus));
  return planner(n, cus, &p->rt, &p->chunks, &p->per);
}

#endif  // DAD_PAIRWISE_H_
