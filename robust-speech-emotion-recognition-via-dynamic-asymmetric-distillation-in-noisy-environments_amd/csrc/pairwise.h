// The n x n pass over the fp32 Gram block of two 64-row tiles of centred embeddings, and everything around it, shared
// by the class-separation pass (cluster.hip), the t-SNE affinities (tsne.hip), the domain gap (domain_gap.hip) and the
// k-NN (knn.hip); scl.hip uses the operand layout and the plan.  One definition of each piece, so the evaluators
// produce the same bits from the same rows:
//
//   before the walk   dad_pair_prep<G, Group, WEIGHTS> (a tile's per-group column sums, counts and non-finite rows),
//                     dad_pair_reduce<G> (the tiles in tile order -> sums, counts, mean, centroids), dad_pair_mean
//                     (dad_pair_reduce<1> into a header), dad_pair_norms (the diagonal of the Gram block) and the
//                     host's pair_centre, which launches the three.  The kernels are defined in pairwise.hip.
//   the walk          the operand layout, the column tile's staging, the MFMA chain, dad_gram_walk over column tiles
//                     t0, t0 + step, ... and dad_gram_walk_chunk over a plan's chunk, and dad_pair_d2
//   behind the walk   flush_bins<W> (a lane's bins -> [64][W] per workgroup), dad_chunk_sum4 (a row's partials in
//                     chunk order) and dad_row_compactness (|x_i - centroid|^2 in double by one wave)
//   on the host       pair_plan, pair_plan_out, pair_plan_resident2 and pair_resolve
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

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// ---------------------------------------------------------------------------------- before the walk
// A row's group: a functor of the row index i < n that returns the group in [0, G), or -1 for a row that takes no part.
__device__ __forceinline__ int class_of(long lab) { return lab >= 0 && lab < DAD_C ? (int)lab : -1; }

struct PairEveryRow {                      // t-SNE: one group, every row
  __device__ __forceinline__ int operator()(int) const { return 0; }
};
struct PairInt32Group {                    // knn: one group, the rows with group[i] >= 0 (every row for NULL)
  const int32_t* group;
  __device__ __forceinline__ int operator()(int i) const { return group && group[i] < 0 ? -1 : 0; }
};
struct PairClassGroup {                    // cluster: the row's class
  const int64_t* labels;
  __device__ __forceinline__ int operator()(int i) const { return class_of(labels[i]); }
};
struct PairDomainGroup {                   // domain gap: 2 * class + domain
  const int64_t* labels;
  const uint8_t* domain;
  __device__ __forceinline__ int operator()(int i) const {
    const long lab = labels[i];
    return lab >= 0 && lab < DAD_C ? 2 * (int)lab + (domain[i] != 0) : -1;
  }
};

// One workgroup per 64-row tile, kGramThreads threads (thread = column): csum[tile][G][256] the per-group column sums
// in double, in row order; cnt[tile][G + 1] the rows per group and, last, the participating rows with a non-finite
// component; for WEIGHTS wsum[tile][G] the groups' weight sums in row order (weights NULL: every weight is 1).  A row
// that takes no part adds to nothing: its NaNs stay out.  Defined and instantiated in pairwise.hip.
template <int G, typename Group, bool WEIGHTS>
__global__ void dad_pair_prep(const float* __restrict__ emb, Group group, const float* __restrict__ weights, int n,
                              double* __restrict__ csum, int32_t* __restrict__ cnt, double* __restrict__ wsum);
extern template __global__ void dad_pair_prep<1, PairEveryRow, false>(const float*, PairEveryRow, const float*, int,
                                                                      double*, int32_t*, double*);
extern template __global__ void dad_pair_prep<1, PairInt32Group, false>(const float*, PairInt32Group, const float*,
                                                                        int, double*, int32_t*, double*);
extern template __global__ void dad_pair_prep<DAD_C, PairClassGroup, false>(const float*, PairClassGroup, const float*,
                                                                            int, double*, int32_t*, double*);
extern template __global__ void dad_pair_prep<2 * DAD_C, PairDomainGroup, true>(const float*, PairDomainGroup,
                                                                                const float*, int, double*, int32_t*,
                                                                                double*);

// What dad_pair_prep's tiles add up to, for column tid of kGramThreads: the group sums s and counts nc over the tiles
// in tile order, the centroids mc = s / nc (0 for an empty group), bad rows, m = sum nc, and the participating rows'
// mean mu = (sum_k s[k]) / m in double and rounded to fp32 (0 for m = 0).
template <int G>
struct PairStats {
  double s[G], mc[G], mu;
  int nc[G], bad, m;
  float mean;
};

// (cent [G][256] or NULL.  The groups' sums are added in group order from s[0]: no s[k] is -0.0, since every
// accumulator starts at +0.0, so ((s0 + s1) + s2) + ... and tot = 0.0, tot += s[k] round identically, and for G = 1
// both are s[0].)
template <int G>
__device__ __forceinline__ PairStats<G> dad_pair_reduce(const double* __restrict__ csum,
                                                        const int32_t* __restrict__ cnt, int rt, int tid,
                                                        double* __restrict__ cent) {
  PairStats<G> p;
#pragma unroll
  for (int k = 0; k < G; ++k) {
    p.s[k] = 0.0;
    p.nc[k] = 0;
  }
  p.bad = 0;
  for (int t = 0; t < rt; ++t) {
#pragma unroll
    for (int k = 0; k < G; ++k) {
      p.s[k] += csum[((size_t)t * G + k) * DAD_H + tid];
      p.nc[k] += cnt[t * (G + 1) + k];
    }
    p.bad += cnt[t * (G + 1) + G];
  }
  p.m = 0;
  double tot = p.s[0];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    p.m += p.nc[k];
    if (k > 0) tot += p.s[k];
    p.mc[k] = p.nc[k] > 0 ? p.s[k] / (double)p.nc[k] : 0.0;
    if (cent) cent[k * DAD_H + tid] = p.mc[k];
  }
  p.mu = p.m > 0 ? tot / (double)p.m : 0.0;
  p.mean = (float)p.mu;
  return p;
}

// dad_pair_reduce<1> and nothing more: mean[256], hdr[kPairHdrBad] the bad rows, hdr[kPairHdrM] the rows.  One
// workgroup of kGramThreads.
constexpr int kPairHdrBad = 0, kPairHdrM = 1;
__global__ void dad_pair_mean(const double* __restrict__ csum, const int32_t* __restrict__ cnt, int rt,
                              float* __restrict__ mean, int32_t* __restrict__ hdr);

// |x_i - mu|^2 per row as the diagonal of the Gram block; norms has ceil(n / 64) * 64 entries, padding rows get 0.
// Grid ceil(n / 64), 128 threads.
__global__ void dad_pair_norms(const float* __restrict__ emb, const float* __restrict__ mean, int n,
                               float* __restrict__ norms);

// What every walk starts from: the prep of G groups over rt tiles, the caller's stats kernel (`stats()` launches it:
// one workgroup that turns csum and cnt into mean, through dad_pair_reduce), and the norms.
template <int G, bool WEIGHTS, typename Group, typename Stats>
inline int pair_centre(const float* emb, Group group, const float* weights, int64_t n, int rt, double* csum,
                       int32_t* cnt, double* wsum, const float* mean, float* norms, hipStream_t stream, Stats stats) {
  hipLaunchKernelGGL((dad_pair_prep<G, Group, WEIGHTS>), dim3(rt), dim3(kGramThreads), 0, stream, emb, group, weights,
                     (int)n, csum, cnt, wsum);
  DAD_TRY(hipGetLastError());
  stats();
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_pair_norms, dim3(rt), dim3(128), 0, stream, emb, mean, (int)n, norms);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

// ---------------------------------------------------------------------------------- the walk

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
// the caller's epi leaves them out.  norms is read unguarded: it has 64 * ceil(n / 64) entries and dad_pair_norms
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

// the walk of column chunk `chunk` of a plan: tiles chunk * per .. min((chunk + 1) * per, ct), one by one
template <typename Extra, typename Epi>
__device__ __forceinline__ void dad_gram_walk_chunk(const float* __restrict__ emb, const float* __restrict__ norms,
                                                    const float* __restrict__ mean, int n, int i0, int chunk, int per,
                                                    int ct, float* __restrict__ bt, float* __restrict__ nj_s,
                                                    float* __restrict__ ni_s, Extra extra, Epi epi) {
  const int t_end = (chunk + 1) * per < ct ? (chunk + 1) * per : ct;
  dad_gram_walk(emb, norms, mean, n, i0, chunk * per, t_end, 1, bt, nj_s, ni_s, extra, epi);
}

// ---------------------------------------------------------------------------------- behind the walk
// the W bins of a lane's 16 rows -> out[row][W] of the workgroup's 64 rows: the 32 columns of a lane half by a fixed xor
// tree, the two column halves through LDS (red: 2 * 64 * W floats, the walk's column tile, behind a barrier)
template <int W>
__device__ __forceinline__ void flush_bins(float (&bins)[16][W], const GramLane& g, float* __restrict__ red,
                                           float* __restrict__ out) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int c = 0; c < W; ++c) {
      float v = bins[r][c];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      bins[r][c] = v;
    }
  __syncthreads();        // the last tile's operand reads are done
  if (g.l32 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int il = 32 * g.rh + dad_acc_row(r, g.kh);
#pragma unroll
      for (int c = 0; c < W; ++c) red[(g.ch * kGramTile + il) * W + c] = bins[r][c];
    }
  }
  __syncthreads();
  const int tid = threadIdx.x;
  static_assert(kGramTile * W <= kGramThreads, "one output per thread");
  if (kGramTile * W == kGramThreads || tid < kGramTile * W)      // (W = 4: every thread, and no compare)
    out[tid] = red[tid] + red[kGramTile * W + tid];
}

// sum[0 .. 3] += the chunks' f32x4 partials part[chunk][npad][4] of row i, in chunk order
__device__ __forceinline__ void dad_chunk_sum4(float (&sum)[4], const float* __restrict__ part, int chunks, int npad,
                                               int i) {
  for (int q = 0; q < chunks; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + ((size_t)q * npad + i) * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] += v[k];
  }
}

// |x - c|^2 of the row x[256] and the centroid c[256] in double by one wave (lane = 4 columns); every lane gets it
__device__ __forceinline__ double dad_row_compactness(const float* __restrict__ x, const double* __restrict__ c,
                                                      int lane) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * lane);
  const double* mu = c + 4 * lane;
  double p = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double d = (double)v[e] - mu[e];
    p += d * d;
  }
  return dad_wave_sum_d(p);
}

// ---------------------------------------------------------------------------------- on the host
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

// a planner's answer
inline int pair_plan_out(const PairPlan& p, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  *row_tiles = p.rt;
  *chunks = p.chunks;
  *tiles_per_chunk = p.per;
  return DAD_OK;
}

// dad_cluster_plan and dad_domain_gap_plan: two workgroups of a pass fit a CU (65 KB of LDS each), so the most chunks
// whose grid is still resident at once (rounding up instead left 5,531 rows on 256 CUs a second round of 10
// workgroups as long as the first of 512)
inline int pair_plan_resident2(int64_t n, int cus, int64_t max_n, int max_chunks, int* row_tiles, int* chunks,
                               int* tiles_per_chunk) {
  if (!row_tiles || !chunks || !tiles_per_chunk) return DAD_E_ARG;
  if (n < 1 || n > max_n || cus < 1) return DAD_E_SHAPE;
  const int rt = (int)((n + kGramTile - 1) / kGramTile);
  return pair_plan_out(pair_plan(n, 2 * cus / rt, max_chunks), row_tiles, chunks, tiles_per_chunk);
}

// the plan of `chunks` asked-for chunks, or for chunks <= 0 the planner's (planner(n, cus, &rt, &chunks, &per): a
// dad_*_plan, or a closure over its further arguments) for the current device
template <typename Planner>
inline int pair_resolve(int64_t n, int chunks, int max_chunks, Planner planner, PairPlan* p) {
  if (chunks > 0) {
    *p = pair_plan(n, chunks, max_chunks);
    return DAD_OK;
  }
  int cus = 0;
  DAD_RET(device_cus(&cus));
  return planner(n, cus, &p->rt, &p->chunks, &p->per);
}

#endif  // DAD_PAIRWISE_H_
