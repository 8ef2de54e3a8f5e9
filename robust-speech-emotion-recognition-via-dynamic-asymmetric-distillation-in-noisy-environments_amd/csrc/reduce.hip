// ---------------------------------------------------------------- reduce + squared norms
// blocks [0, NB): DAD_REDUCE_COLS floats of dW1 each (+ squared-norm partial).
// blocks NB + e, e < DAD_REDUCE_XBLK: the extra blocks (extra_block, wgrad_common.h)
#include "wgrad_common.h"

static_assert(DAD_REDUCE_THREADS == 4 * (DAD_REDUCE_COLS / 4), "dad_reduce: 4 split groups x float4 columns");
static_assert(DAD_REDUCE_BLOCKS <= DAD_NORM_BLOCKS, "norm partials must fit the workspace");
static_assert((DAD_NPARAM + 1023) / 1024 <= DAD_NORM_BLOCKS, "dad_norm partials must fit the workspace");
__global__ __launch_bounds__(DAD_REDUCE_THREADS) void dad_reduce(DadReduceArgs a) {
  DAD_GUARD_BLOCK(DAD_REDUCE_THREADS);
  __shared__ double red[DAD_REDUCE_THREADS / 64];
  __shared__ f32x4 part[4][DAD_REDUCE_COLS / 4 > DAD_H / 4 ? DAD_REDUCE_COLS / 4 : DAD_H / 4];
  const int tid = threadIdx.x;
  constexpr int NB = DAD_REDUCE_BLOCKS - DAD_REDUCE_XBLK;
  double sq = 0.0;
  if (blockIdx.x < NB) {
    const int col = tid & (DAD_REDUCE_COLS / 4 - 1), kg = tid / (DAD_REDUCE_COLS / 4);
    const size_t e0 = (size_t)blockIdx.x * DAD_REDUCE_COLS + (size_t)col * 4;
    f32x4 s = f32x4{};
#pragma unroll 4
    for (int k = kg; k < a.splits; k += 4) s += *reinterpret_cast<const f32x4*>(a.wpart + (size_t)k * DAD_H * DAD_D + e0);
    part[kg][col] = s;
    __syncthreads();
    if (kg == 0) {
      const f32x4 t = ((part[0][col] + part[1][col]) + part[2][col]) + part[3][col];
      *reinterpret_cast<f32x4*>(a.grad + DAD_OFF_W1 + e0) = t;
      for (int e = 0; e < 4; ++e) sq += (double)t[e] * t[e];
    }
  } else {
    __shared__ float xsx[16][16][6];
    sq = extra_block(a, blockIdx.x - NB, tid, xsx);
  }
  if (!a.want_norm) return;
  double v = dad_wave_sum_d(sq);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < DAD_REDUCE_THREADS / 64; ++k) t += red[k];
    a.normpart[blockIdx.x] = (float)t;
  }
}

// FP16/BF16 step (the extra blocks ran on spare dad_wgrad_direct workgroups): one wave per
// DAD_REDUCE_COLS columns, 4 per lane, the splits summed in split order with every partial's
// load issued first (batches of 8, index clamped, +0 past the last split), the squared-norm
// partial a wave reduction: no LDS, no barrier (dad_reduce's 4 row groups met through LDS
// twice).
static_assert(DAD_REDUCE_COLS == 4 * 64, "dad_reduce_w: one wave, 4 columns per lane");
__global__ __launch_bounds__(64) void dad_reduce_w(DadReduceArgs a) {
  DAD_GUARD_BLOCK(64);
  const int lane = threadIdx.x;
  const size_t e0 = (size_t)blockIdx.x * DAD_REDUCE_COLS + 4 * (size_t)lane;
  constexpr int KB = 8;
  f32x4 t = f32x4{};
  for (int k0 = 0; k0 < a.splits; k0 += KB) {
    f32x4 v[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k)
      v[k] = *reinterpret_cast<const f32x4*>(a.wpart + (size_t)min(k0 + k, a.splits - 1) * DAD_H * DAD_D + e0);
#pragma unroll
    for (int k = 0; k < KB; ++k) t += k0 + k < a.splits ? v[k] : f32x4{};
  }
  *reinterpret_cast<f32x4*>(a.grad + DAD_OFF_W1 + e0) = t;
  if (!a.want_norm) return;
  double sq = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) sq += (double)t[e] * t[e];
  sq = dad_wave_sum_d(sq);
  if (lane == 0) a.normpart[blockIdx.x] = (float)sq;
}

// Data-parallel path: after the SUM all-reduce, average (grads, thresholds, losses) and
// recompute the squared-norm partials over the averaged gradient.
__global__ __launch_bounds__(256) void dad_norm(float* grad, float* normpart, float inv) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double sq = 0.0;
  const size_t n0 = (size_t)blockIdx.x * 1024;
  for (int k = 0; k < 4; ++k) {
    const size_t e = n0 + (size_t)k * 256 + tid;
    if (e < DAD_NPARAM) {
      const float g = grad[e] * inv;
      grad[e] = g;
      sq += (double)g * g;
    }
  }
  if (blockIdx.x == 0 && tid < DAD_GRAD_EXTRA) {
    float* ex = grad + DAD_NPARAM;
    if (tid < 4 || tid >= 12) ex[tid] *= inv;   // thresholds and losses are means; sums stay sums
  }
  double v = dad_wave_sum_d(sq);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) normpart[blockIdx.x] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}
