// The fp32 Gram block of two 64-row tiles of centred embeddings, shared by the class-separation pass (cluster.hip)
// and the t-SNE affinities (tsne.hip): one definition of the operand layout, the column tile's staging and the MFMA
// chain, so both passes (and dad_cluster_norms, the diagonal of the same block) produce the same bits from the same
// rows.
//
//   A operand   row ia of the row tile, lane = row (l32), 4 consecutive k per k-block of 8 and lane half (kh):
//               MFMA step e of k-block q takes k = 8 q + 4 kh + e on both operands
//   B operand   the column tile's rows in LDS, row stride kGramLd = 260 floats (the 16-byte operand reads of 8
//               consecutive rows cover the 32 banks once)
//   result      acc[r] = (x_row - mu).(x_col - mu), row = dad_acc_row(r, kh) of the wave's 32 rows, col = l32
#ifndef DAD_CLUSTER_GRAM_H_
#define DAD_CLUSTER_GRAM_H_
#include "dad_common.h"

constexpr int kGramTile = 64;              // rows and columns of a tile
constexpr int kGramLd = DAD_H + 4;         // LDS row stride of the column tile, floats
constexpr int kGramThreads = 256;          // 4 waves: (row half, column half) quadrants of 32 x 32

// |x_i - mu|^2 per row as the diagonal of the Gram block (cluster.hip); norms has ceil(n / 64) * 64 entries, padding
// rows get 0.  Grid ceil(n / 64), 128 threads.
__global__ void dad_cluster_norms(const float* __restrict__ emb, const float* __restrict__ mean, int n,
                                  float* __restrict__ norms);

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

#endif  // DAD_CLUSTER_GRAM_H_
