// The kernels every pairwise evaluator (cluster.hip, tsne.hip, domain_gap.hip, knn.hip) launches before its walk of the
// Gram block; pairwise.h declares them and holds the device functions they share with the evaluators' own kernels.
//
//   dad_pair_prep<G, Group, WEIGHTS>   one workgroup per 64-row tile: the tile's per-group column sums in double, its
//                                      group counts (and weight sums), its count of participating rows with a
//                                      non-finite component.  Instantiated for the four evaluators' group functors.
//   dad_pair_mean                      one workgroup: the tiles of a one-group prep in tile order -> the participating
//                                      rows' mean rounded to fp32, the bad rows and the row count into a header
//   dad_pair_norms                     |x_i - mu|^2 per row, as the diagonal of the walk's own Gram block
#include <cstdint>

#include "dad_common.h"
#include "pairwise.h"

static_assert(kGramTile == 64 && kGramThreads == DAD_H, "thread = column of the embeddings; one wave per row in turn");

// Non-finite rows are found by a wave per row (a ballot over f32x4 loads) ahead of the column loop, which stays a
// load, a convert and G select-adds.  With one group the tile would be read a second time for nothing: there the
// column loop tests the value it has already loaded (kInLoop; on the MI355X the ballot form cost dad_tsne_affinities
// 4 us of 189 at n = 1,100, beyond the 2 to 4 us its repeated runs spread over).  Either way bad_s[r] is
// 1 exactly for a participating row with a non-finite component.  With one group every participating row has g == 0,
// so the select-add is s[0] += x: the bits of a plain column sum.
template <int G, typename Group, bool WEIGHTS>
__global__ __launch_bounds__(kGramThreads) void dad_pair_prep(const float* __restrict__ emb, Group group,
                                                              const float* __restrict__ weights, int n,
                                                              double* __restrict__ csum, int32_t* __restrict__ cnt,
                                                              double* __restrict__ wsum) {
  __shared__ int g_s[kGramTile], bad_s[kGramTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, i0 = kGramTile * tile;
  constexpr bool kInLoop = G == 1;
  if (tid < kGramTile) {
    g_s[tid] = i0 + tid < n ? group(i0 + tid) : -1;
    if constexpr (kInLoop) bad_s[tid] = 0;
  }
  __syncthreads();
  if constexpr (!kInLoop) {
    for (int rr = w; rr < kGramTile; rr += kGramThreads / 64) {
      const int i = i0 + rr;           // (uniform in the wave)
      bool bad = false;
      if (i < n) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(emb + (size_t)i * DAD_H + 4 * lane);
        bad = __ballot(nonfinite(v[0]) | nonfinite(v[1]) | nonfinite(v[2]) | nonfinite(v[3])) != 0ull;
      }
      if (lane == 0) bad_s[rr] = bad && g_s[rr] >= 0;
    }
  }
  double s[G];
#pragma unroll
  for (int k = 0; k < G; ++k) s[k] = 0.0;
  const int rows = n - i0 < kGramTile ? n - i0 : kGramTile;
  for (int rr = 0; rr < rows; ++rr) {
    const int g = g_s[rr];
    if (g < 0) continue;             // (a row that takes no part is not read: its NaNs stay out)
    const float xf = emb[(size_t)(i0 + rr) * DAD_H + tid];
    if constexpr (kInLoop)
      if (nonfinite(xf)) bad_s[rr] = 1;
    const double x = (double)xf;
#pragma unroll
    for (int k = 0; k < G; ++k) s[k] += g == k ? x : 0.0;
  }
#pragma unroll
  for (int k = 0; k < G; ++k) csum[((size_t)tile * G + k) * DAD_H + tid] = s[k];
  __syncthreads();
  if (tid < G) {
    int v = 0;
    double ws = 0.0;
    for (int rr = 0; rr < rows; ++rr)
      if (g_s[rr] == tid) {
        v += 1;
        if constexpr (WEIGHTS) ws += weights ? (double)weights[i0 + rr] : 1.0;
      }
    cnt[tile * (G + 1) + tid] = v;
    if constexpr (WEIGHTS) wsum[tile * G + tid] = ws;
  } else if (tid == G) {
    int v = 0;
    for (int rr = 0; rr < kGramTile; ++rr) v += bad_s[rr];
    cnt[tile * (G + 1) + G] = v;
  }
}

template __global__ void dad_pair_prep<1, PairEveryRow, false>(const float*, PairEveryRow, const float*, int, double*,
                                                               int32_t*, double*);
template __global__ void dad_pair_prep<1, PairInt32Group, false>(const float*, PairInt32Group, const float*, int,
                                                                 double*, int32_t*, double*);
template __global__ void dad_pair_prep<DAD_C, PairClassGroup, false>(const float*, PairClassGroup, const float*, int,
                                                                     double*, int32_t*, double*);
template __global__ void dad_pair_prep<2 * DAD_C, PairDomainGroup, true>(const float*, PairDomainGroup, const float*,
                                                                         int, double*, int32_t*, double*);

__global__ __launch_bounds__(kGramThreads) void dad_pair_mean(const double* __restrict__ csum,
                                                              const int32_t* __restrict__ cnt, int rt,
                                                              float* __restrict__ mean, int32_t* __restrict__ hdr) {
  const int tid = threadIdx.x;
  const PairStats<1> p = dad_pair_reduce<1>(csum, cnt, rt, tid, nullptr);
  mean[tid] = p.mean;
  if (tid == 0) {
    hdr[kPairHdrBad] = p.bad;
    hdr[kPairHdrM] = p.m;
  }
}

// |x_i - mu|^2 as the diagonal of the walk's own Gram block: the same operand values through the same chain of 128
// MFMAs, so (x_i - mu).(x_j - mu) of an exact duplicate j equals it bit for bit and their distance is exactly 0.  One
// wave per 32 rows.
__global__ __launch_bounds__(128) void dad_pair_norms(const float* __restrict__ emb, const float* __restrict__ mean,
                                                      int n, float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int kh = lane >> 5, l32 = lane & 31;
  const int r0 = kGramTile * (int)blockIdx.x + 32 * w, ia = r0 + l32;
  const float* ra = emb + (size_t)(ia < n ? ia : 0) * DAD_H + 4 * kh;
  f32x16 acc = f32x16{};
#pragma unroll 4
  for (int q = 0; q < DAD_H / 8; ++q) {
    const f32x4 v = ia < n ? *reinterpret_cast<const f32x4*>(ra + 8 * q) -
                                 *reinterpret_cast<const f32x4*>(mean + 4 * kh + 8 * q)
                           : f32x4{};
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], v[e], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (l32 == dad_acc_row(r, kh)) norms[r0 + l32] = acc[r];   // (rt * 64 entries: padding rows get 0)
}
