// Exact t-SNE of a split's embeddings on the device, with scikit-learn 1.7.2's meaning (method='exact').
//
// Replaces run_tsne (I/iemocap_plot_tsne.py:310-323).  Three stages, as scikit-learn splits them (include/dad.h
// restates the arithmetic); no floating-point atomics, every sum in a fixed order:
//
//   dad_tsne_affinities   _joint_probabilities
//     dad_pair_prep       (pairwise.hip, one group: every row) one workgroup per 64-row tile: the tile's column sums
//                         in double, its count of rows with a non-finite component
//     dad_pair_mean       (pairwise.hip) one workgroup: the tiles in tile order -> the rows' mean rounded to fp32, the
//                         count into the workspace's first word
//     dad_pair_norms      (pairwise.hip) |x_i - mu|^2 as the diagonal of the Gram block
//     dad_tsne_dist       pairwise.h's walk of the Gram block per 64 x 64 tile -> D_ij = dad_pair_d2
//                         into P (D_ii = 0; a duplicate row's distance is exactly 0)
//     dad_tsne_search     one wave per row: scikit-learn's _binary_search_perplexity in double on the row's fp32
//                         distances; the row's conditional probabilities replace its distances
//     dad_tsne_sym        one workgroup per tile pair (ti <= tj): s_ij = c_ij + c_ji into both tiles (the same bits),
//                         the tile's sum in double
//     dad_tsne_total      one workgroup: the tile sums in tile order
//     dad_tsne_scale      P_ij = max(s_ij / max(sum, eps), eps), P_ii = 0, padding columns 0
//   dad_tsne_gradient     _kl_divergence (one degree of freedom)
//     dad_tsne_force      the n x n pass.  Workgroup (row tile of 64, column chunk); lane = row, holding y_i and its five
//                         running sums in registers; each of the 4 waves takes a quarter of every staged block of the
//                         chunk's columns, whose y_j sit in LDS.  P is bit-symmetric, so lane i reads P[j][i]: one
//                         256-byte run per column and wave.  The waves meet in LDS in wave order and the workgroup
//                         writes its sums [chunk][5][row] to the workspace.  The <true> instance also sums
//                         P (log P - log w) and P per row in double (the error, every 50th iteration).
//     dad_tsne_step       one workgroup: the chunks in chunk order -> Z, the gradient, its norm, the error; the
//                         <true> instance then applies _gradient_descent's update and stop rules
//   dad_tsne_run          TSNE._tsne: dad_tsne_init, then max_iter x (dad_tsne_force, dad_tsne_step<true>).  The phase, the
//                         best error and the stop flag live in a device header; after a stop every launch returns at
//                         its entry.  The host never reads anything back.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "dad_common.h"
#include "pairwise.h"

namespace {

constexpr int kTile = DAD_TS_TILE;
constexpr int kMaxChunks = DAD_TS_MAX_CHUNKS;
constexpr int kThreads = kGramThreads;
constexpr int kStage = 2048;               // y_j staged per block of a chunk's columns
#ifndef DAD_TS_UNROLL
#define DAD_TS_UNROLL 8
#endif
constexpr int kUnroll = DAD_TS_UNROLL;     // P loads in flight per lane in the force kernel's column loop
constexpr int kStepThreads = 1024;
constexpr int kCheck = 50;                 // _gradient_descent's n_iter_check
constexpr int kExplore = 250;              // TSNE._EXPLORATION_MAX_ITER
constexpr double kEps = 2.220446049250313e-16;

static_assert(kTile == kGramTile && kTile == 64 && DAD_H == 256, "the Gram block's wave / lane mapping");
static_assert(DAD_TS_WS_NONFINITE == kPairHdrBad, "dad_pair_mean writes the count where include/dad.h promises it");

struct RunHdr {
  int32_t stop, phase, best_iter, nhist;
  double best_error, last_error;
};

struct TsneWs {
  size_t hdr, mean, norms, csum, cnt, tsum, total, part, partd, upd, gains, bytes;
};

// (a function of n alone)
TsneWs tsne_ws_layout(int64_t n) {
  TsneWs w;
  const size_t rt = (size_t)((n + kTile - 1) / kTile), npad = rt * kTile;
  const size_t maxc = rt < (size_t)kMaxChunks ? rt : (size_t)kMaxChunks;
  size_t off = 0;
  w.hdr = off;    off = dad_align(off + 256);        // int32 [0]: DAD_TS_WS_NONFINITE, [1]: n; RunHdr at byte 64
  w.mean = off;   off = dad_align(off + sizeof(float) * DAD_H);
  w.norms = off;  off = dad_align(off + sizeof(float) * npad);
  w.csum = off;   off = dad_align(off + sizeof(double) * rt * DAD_H);
  w.cnt = off;    off = dad_align(off + sizeof(int32_t) * rt * 2);
  w.tsum = off;   off = dad_align(off + sizeof(double) * rt * rt);
  w.total = off;  off = dad_align(off + sizeof(double) * 2);
  w.part = off;   off = dad_align(off + sizeof(float) * maxc * 5 * npad);
  w.partd = off;  off = dad_align(off + sizeof(double) * maxc * 2 * npad);
  w.upd = off;    off = dad_align(off + sizeof(float) * 2 * npad);
  w.gains = off;  off = dad_align(off + sizeof(float) * 2 * npad);
  w.bytes = off;
  return w;
}

// the sum of v over the workgroup's kStepThreads threads in a fixed order (each wave's fixed DPP tree, then the waves
// in wave order); every thread gets it
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  v = dad_wave_sum_d(v);
  __syncthreads();        // the previous sum's reads are done
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kStepThreads / 64; ++w) s += red[w];
  return s;
}

}  // namespace

// ---------------------------------------------------------------------------------- affinities
// D_ij into P for i, j < n.  Grid (row tiles, y): workgroup (x, y) takes the column tiles y, y + gridDim.y, ...
__global__ __launch_bounds__(kThreads, 2) void dad_tsne_dist(const float* __restrict__ emb,
                                                             const float* __restrict__ norms,
                                                             const float* __restrict__ mean, int n, int ct, int ld,
                                                             float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ float nj_s[kTile], ni_s[kTile];
  dad_gram_walk(
      emb, norms, mean, n, kTile * (int)blockIdx.x, blockIdx.y, ct, gridDim.y, bt, nj_s, ni_s, [](int, int) {},
      [&](int, int ig, int, int jg, float d2) {
        if (ig < n && jg < n) P[(size_t)ig * ld + jg] = d2;
      });
}

// _binary_search_perplexity of one row per wave.  The row of P holds D_i. on entry and the conditional c_i. on exit.
__global__ __launch_bounds__(kThreads) void dad_tsne_search(float* __restrict__ P, int n, int ld, double desired,
                                                            double* __restrict__ beta_out) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int row = 4 * (int)blockIdx.x + w;
  if (row >= n) return;                    // (uniform in the wave)
  float* prow = P + (size_t)row * ld;
  const double tol = (double)1e-5f, tiny = (double)1e-8f;   // (scikit-learn holds both as C floats)
  double beta = 1.0, bmin = -INFINITY, bmax = INFINITY, used = 1.0, sum = 1.0;
  for (int l = 0; l < 100; ++l) {
    double s = 0.0, sd = 0.0;
    for (int j = lane; j < n; j += 64) {
      const double d = (double)prow[j];
      const double e = j == row ? 0.0 : exp(-d * beta);
      s += e;
      sd += d * e;
    }
    s = dad_wave_sum_d(s);
    sd = dad_wave_sum_d(sd);
    if (s == 0.0) s = tiny;
    used = beta;
    sum = s;
    const double diff = (log(s) + beta * (sd / s)) - desired;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      bmin = beta;
      beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) / 2.0;
    } else {
      bmax = beta;
      beta = bmin == -INFINITY ? beta / 2.0 : (beta + bmin) / 2.0;
    }
  }
  for (int j = lane; j < n; j += 64) {
    const double d = (double)prow[j];
    prow[j] = j == row ? 0.0f : (float)(exp(-d * used) / sum);
  }
  if (lane == 0 && beta_out) beta_out[row] = used;
}

// s_ij = c_ij + c_ji of the tile pair (ti, tj), ti <= tj, in place; tsum[ti * ct + tj] = the sum over tile (ti, tj)
__global__ __launch_bounds__(kThreads) void dad_tsne_sym(float* __restrict__ P, int n, int ld, int ct,
                                                         double* __restrict__ tsum) {
  __shared__ float A[kTile][kTile + 1], B[kTile][kTile + 1];
  __shared__ double red[kThreads];
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  if (ti > tj) return;
  const int i0 = kTile * ti, j0 = kTile * tj;
#pragma unroll 4
  for (int e = 0; e < kTile * kTile / kThreads; ++e) {
    const int idx = tid + kThreads * e, r = idx >> 6, c = idx & 63;
    A[r][c] = i0 + r < n && j0 + c < n ? P[(size_t)(i0 + r) * ld + j0 + c] : 0.0f;
    B[r][c] = j0 + r < n && i0 + c < n ? P[(size_t)(j0 + r) * ld + i0 + c] : 0.0f;
  }
  __syncthreads();
  double acc = 0.0;
#pragma unroll 4
  for (int e = 0; e < kTile * kTile / kThreads; ++e) {
    const int idx = tid + kThreads * e, r = idx >> 6, c = idx & 63;
    const float sa = A[r][c] + B[c][r];
    if (i0 + r < n && j0 + c < n) P[(size_t)(i0 + r) * ld + j0 + c] = sa;
    acc += (double)sa;
    if (ti != tj) {
      const float sb = B[r][c] + A[c][r];
      if (j0 + r < n && i0 + c < n) P[(size_t)(j0 + r) * ld + i0 + c] = sb;
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int d = 0; d < kThreads; ++d) s += red[d];
    tsum[(size_t)ti * ct + tj] = s;
  }
}

__global__ __launch_bounds__(kThreads) void dad_tsne_total(const double* __restrict__ tsum, int ct,
                                                           double* __restrict__ total) {
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int k = tid; k < ct * ct; k += kThreads) {
    const int ti = k / ct, tj = k - ti * ct;
    if (ti <= tj) acc += (ti < tj ? 2.0 : 1.0) * tsum[k];
  }
  red[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int d = 0; d < kThreads; ++d) s += red[d];
    total[0] = s > kEps ? s : kEps;
  }
}

__global__ __launch_bounds__(kThreads) void dad_tsne_scale(float* __restrict__ P, int n, int ld,
                                                           const double* __restrict__ total) {
  const int i = blockIdx.x;
  const double sum = total[0];
  float* prow = P + (size_t)i * ld;
  for (int j = threadIdx.x; j < ld; j += kThreads) {
    const float v = fmaxf((float)((double)prow[j] / sum), (float)kEps);
    prow[j] = j >= n || j == i ? 0.0f : v;
  }
}

// ---------------------------------------------------------------------------------- one evaluation
struct TsneForceArgs {
  const float* P;
  const float* Y;
  float* part;          // [chunks][5][npad]: sum p w dy (2), sum w^2 dy (2), sum w
  double* partd;        // [chunks][2][npad]: sum P (log P - log w), sum P
  const int32_t* stop;  // the run's stop flag, or NULL
  int n, npad, ld, per;
};

template <bool KL>
__global__ __launch_bounds__(kThreads) void dad_tsne_force(TsneForceArgs a) {
  __shared__ f32x2 ys[kStage];
  __shared__ float red[3][5][kTile];
  __shared__ double redd[KL ? 3 : 1][2][kTile];
  if (a.stop && *a.stop) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n, chunk = blockIdx.y;
  const int i = kTile * (int)blockIdx.x + lane;
  const f32x2* Y2 = reinterpret_cast<const f32x2*>(a.Y);
  const f32x2 yi = i < n ? Y2[i] : f32x2{0.0f, 0.0f};
  float ax = 0.0f, ay = 0.0f, rx = 0.0f, ry = 0.0f, z = 0.0f;
  double kl = 0.0, sp = 0.0;
  const int c0 = chunk * a.per * kTile;
  const int c1 = c0 + a.per * kTile < n ? c0 + a.per * kTile : n;
  for (int b0 = c0; b0 < c1; b0 += kStage) {
    const int bn = c1 - b0 < kStage ? c1 - b0 : kStage;
    __syncthreads();      // the previous block's reads are done
    for (int k = tid; k < bn; k += kThreads) ys[k] = Y2[b0 + k];
    __syncthreads();
    const int q = (bn + 3) >> 2;
    const int j0 = w * q, j1 = j0 + q < bn ? j0 + q : bn;
    const float* pp = a.P + (size_t)(b0 + j0) * a.ld + i;      // (i < npad = ld: inside the row's padding)
#pragma unroll kUnroll
    for (int j = j0; j < j1; ++j) {
      const float p = *pp;
      pp += a.ld;
      const f32x2 yj = ys[j];
      const float dx = yi[0] - yj[0], dy = yi[1] - yj[1];
      const float d2 = fmaf(dx, dx, dy * dy);
      float wq = __builtin_amdgcn_rcpf(1.0f + d2);
      wq = b0 + j == i ? 0.0f : wq;
      z += wq;
      const float pw = p * wq, w2 = wq * wq;
      ax = fmaf(pw, dx, ax);
      ay = fmaf(pw, dy, ay);
      rx = fmaf(w2, dx, rx);
      ry = fmaf(w2, dy, ry);
      if constexpr (KL) {
        const double pd = (double)p;
        kl += p > 0.0f ? pd * (log(pd) + log1p((double)d2)) : 0.0;
        sp += pd;
      }
    }
  }
  __syncthreads();
  if (w > 0) {
    red[w - 1][0][lane] = ax; red[w - 1][1][lane] = ay; red[w - 1][2][lane] = rx; red[w - 1][3][lane] = ry;
    red[w - 1][4][lane] = z;
    if constexpr (KL) { redd[w - 1][0][lane] = kl; redd[w - 1][1][lane] = sp; }
  }
  __syncthreads();
  if (w == 0) {
    float v[5] = {ax, ay, rx, ry, z};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      v[k] = ((v[k] + red[0][k][lane]) + red[1][k][lane]) + red[2][k][lane];
      a.part[((size_t)chunk * 5 + k) * a.npad + i] = v[k];
    }
    if constexpr (KL) {
      a.partd[((size_t)chunk * 2 + 0) * a.npad + i] = ((kl + redd[0][0][lane]) + redd[1][0][lane]) + redd[2][0][lane];
      a.partd[((size_t)chunk * 2 + 1) * a.npad + i] = ((sp + redd[0][1][lane]) + redd[1][1][lane]) + redd[2][1][lane];
    }
  }
}

struct TsneStepArgs {
  const float* part;
  const double* partd;
  float* Y;
  float* upd;
  float* gains;
  float* grad;          // [n][2] or NULL
  RunHdr* hdr;
  double* history;
  double* out;
  int n, npad, chunks;
  int it, check, compute, explore_n, max_iter, nwp;
  float lr, early_ex, ex;
  double min_grad_norm;
};

template <bool STEP>
__global__ __launch_bounds__(kStepThreads) void dad_tsne_step(TsneStepArgs a) {
  __shared__ double red[kStepThreads / 64];
  __shared__ int reset_s;
  const int tid = threadIdx.x, n = a.n;
  int phase = 0;
  if constexpr (STEP) {
    if (a.hdr->stop) return;
    phase = a.hdr->phase;
  }
  const float ex = STEP ? (phase == 0 ? a.early_ex : 1.0f) : a.ex;
  const float mom = phase == 0 ? 0.5f : 0.8f;
  const size_t np = (size_t)a.npad;
  double zl = 0.0;
  for (int i = tid; i < n; i += kStepThreads) {
    float s = 0.0f;
#pragma unroll 8
    for (int q = 0; q < a.chunks; ++q) s += a.part[((size_t)q * 5 + 4) * np + i];
    zl += (double)s;
  }
  const double Z = block_sum(zl, red);
  double A = 0.0, S = 0.0;
  if (a.compute) {
    double k = 0.0, sp = 0.0;
    for (int i = tid; i < n; i += kStepThreads)
#pragma unroll 4
      for (int q = 0; q < a.chunks; ++q) {
        k += a.partd[((size_t)q * 2 + 0) * np + i];
        sp += a.partd[((size_t)q * 2 + 1) * np + i];
      }
    A = block_sum(k, red);
    S = block_sum(sp, red);
  }
  double g2 = 0.0;
  for (int i = tid; i < n; i += kStepThreads) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int q = 0; q < a.chunks; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += a.part[((size_t)q * 5 + k) * np + i];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float g = (float)(4.0 * ((double)ex * (double)s[c] - (double)s[2 + c] / Z));
      if constexpr (STEP) {
        float u = a.upd[2 * i + c], gn = a.gains[2 * i + c];
        gn = u * g < 0.0f ? gn + 0.2f : gn * 0.8f;
        gn = fmaxf(gn, 0.01f);
        g *= gn;
        u = mom * u - a.lr * g;
        a.upd[2 * i + c] = u;
        a.gains[2 * i + c] = gn;
        a.Y[2 * i + c] += u;
      }
      if (a.grad) a.grad[2 * i + c] = g;
      g2 += (double)g * (double)g;
    }
  }
  const double gnorm = sqrt(block_sum(g2, red));
  if (tid == 0) {
    int reset = 0;
    const double exd = (double)ex;
    const double error = a.compute ? exd * (A + log(exd) * S) + log(Z) * (exd * S) : 0.0;
    a.out[DAD_TS_Z] = Z;
    a.out[DAD_TS_GRAD_NORM] = gnorm;
    if (a.compute) a.out[DAD_TS_KL] = error;
    if constexpr (STEP) {
      RunHdr* h = a.hdr;
      bool stop = false;
      if (a.compute) h->last_error = error;
      if (a.check) {
        const int nh = h->nhist;
        a.history[2 * nh] = error;
        a.history[2 * nh + 1] = gnorm;
        h->nhist = nh + 1;
        a.out[DAD_TS_N_CHECKS] = (double)(nh + 1);
        if (error < h->best_error) {
          h->best_error = error;
          h->best_iter = a.it;
        } else if (a.it - h->best_iter > (phase == 0 ? kExplore : a.nwp)) {
          stop = true;
        }
        if (gnorm <= a.min_grad_norm) stop = true;
      }
      if (stop || a.it == (phase == 0 ? a.explore_n : a.max_iter) - 1) {
        if (phase == 0 && a.it + 1 < a.max_iter) {
          h->phase = 1;
          h->best_error = DBL_MAX;
          h->best_iter = a.it + 1;
          reset = 1;
        } else {
          h->stop = 1;
          a.out[DAD_TS_N_ITER] = (double)a.it;
          a.out[DAD_TS_KL] = h->last_error;
        }
      }
    }
    reset_s = reset;
  }
  if constexpr (STEP) {
    __syncthreads();
    if (reset_s)
      for (int k = tid; k < 2 * n; k += kStepThreads) {
        a.upd[k] = 0.0f;
        a.gains[k] = 1.0f;
      }
  }
}

__global__ __launch_bounds__(kStepThreads) void dad_tsne_init(RunHdr* hdr, float* upd, float* gains, double* out, int n) {
  const int tid = threadIdx.x;
  for (int k = tid; k < 2 * n; k += kStepThreads) {
    upd[k] = 0.0f;
    gains[k] = 1.0f;
  }
  if (tid < DAD_TS_SLOTS) out[tid] = tid == DAD_TS_N_ITER ? -1.0 : 0.0;
  if (tid == 0) {
    hdr->stop = 0;
    hdr->phase = 0;
    hdr->best_iter = 0;
    hdr->nhist = 0;
    hdr->best_error = DBL_MAX;
    hdr->last_error = DBL_MAX;
  }
}

namespace {

int launch_force(const float* P, const float* Y, int64_t n, const PairPlan& pl, const TsneWs& L, void* ws, bool kl,
                 const int32_t* stop, hipStream_t stream) {
  TsneForceArgs fa;
  fa.P = P; fa.Y = Y; fa.part = ws_ptr<float>(ws, L.part); fa.partd = ws_ptr<double>(ws, L.partd); fa.stop = stop;
  fa.n = (int)n; fa.npad = pl.rt * kTile; fa.ld = pl.rt * kTile; fa.per = pl.per;
  if (kl) hipLaunchKernelGGL(dad_tsne_force<true>, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, fa);
  else hipLaunchKernelGGL(dad_tsne_force<false>, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, fa);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int dad_tsne_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  if (!row_tiles || !chunks || !tiles_per_chunk) return DAD_E_ARG;
  if (n < 2 || n > DAD_TS_MAX_N || cus < 1) return DAD_E_SHAPE;
  // the force kernel keeps 41 registers and 20 KB of LDS: four workgroups of 256 threads a CU hide the latency of
  // the P reads; a chunk shorter than 4 column tiles (64 columns a wave) is mostly prologue, and every chunk adds
  // 5 n partial sums for the single workgroup of the step launch to read
  const int rt = (int)((n + kTile - 1) / kTile);
  const int want = 4 * cus / rt;
  return pair_plan_out(pair_plan(n, want < rt / 4 ? want : rt / 4, kMaxChunks), row_tiles, chunks, tiles_per_chunk);
}

extern "C" size_t dad_tsne_workspace_bytes(int64_t n) {
  if (n < 2 || n > DAD_TS_MAX_N) return 0;
  return tsne_ws_layout(n).bytes;
}

extern "C" int dad_tsne_affinities(const float* emb, int64_t n, double perplexity, float* P, double* beta,
                                   void* ws, void* stream_) {
  if (!emb || !P || !ws) return DAD_E_ARG;
  if (n < 2 || n > DAD_TS_MAX_N) return DAD_E_SHAPE;
  if (!(perplexity > 0.0) || !(perplexity < (double)n)) return DAD_E_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const TsneWs L = tsne_ws_layout(n);
  const int rt = (int)((n + kTile - 1) / kTile), ld = rt * kTile;
  float *mean = ws_ptr<float>(ws, L.mean), *norms = ws_ptr<float>(ws, L.norms);
  double *csum = ws_ptr<double>(ws, L.csum), *tsum = ws_ptr<double>(ws, L.tsum), *total = ws_ptr<double>(ws, L.total);
  int32_t *cnt = ws_ptr<int32_t>(ws, L.cnt), *hdr = ws_ptr<int32_t>(ws, L.hdr);

  DAD_RET((pair_centre<1, false>(emb, PairEveryRow{}, nullptr, n, rt, csum, cnt, nullptr, mean, norms, stream, [&] {
    hipLaunchKernelGGL(dad_pair_mean, dim3(1), dim3(kThreads), 0, stream, csum, cnt, rt, mean, hdr);
  })));
  hipLaunchKernelGGL(dad_tsne_dist, dim3(rt, rt < 8 ? rt : 8), dim3(kThreads), 0, stream, emb, norms, mean, (int)n, rt, ld, P);
  DAD_TRY(hipGetLastError());
  // (the perplexity as the C float scikit-learn's search receives it)
  hipLaunchKernelGGL(dad_tsne_search, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0, stream, P, (int)n, ld,
                     log((double)(float)perplexity), beta);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_tsne_sym, dim3(rt, rt), dim3(kThreads), 0, stream, P, (int)n, ld, rt, tsum);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_tsne_total, dim3(1), dim3(kThreads), 0, stream, tsum, rt, total);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_tsne_scale, dim3((unsigned)n), dim3(kThreads), 0, stream, P, (int)n, ld, total);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_tsne_gradient_chunked(const float* P, int64_t n, const float* Y, double exaggeration, double* out,
                                         float* grad, int chunks, void* ws, void* stream_) {
  if (!P || !Y || !out || !grad || !ws) return DAD_E_ARG;
  if (n < 2 || n > DAD_TS_MAX_N) return DAD_E_SHAPE;
  if (!(exaggeration > 0.0)) return DAD_E_ARG;
  PairPlan pl;
  DAD_RET(pair_resolve(n, chunks, kMaxChunks, dad_tsne_plan, &pl));
  hipStream_t stream = (hipStream_t)stream_;
  const TsneWs L = tsne_ws_layout(n);
  DAD_RET(launch_force(P, Y, n, pl, L, ws, true, nullptr, stream));
  TsneStepArgs sa = {};
  sa.part = ws_ptr<float>(ws, L.part); sa.partd = ws_ptr<double>(ws, L.partd);
  sa.grad = grad; sa.out = out;
  sa.n = (int)n; sa.npad = pl.rt * kTile; sa.chunks = pl.chunks;
  sa.compute = 1; sa.ex = (float)exaggeration;
  hipLaunchKernelGGL(dad_tsne_step<false>, dim3(1), dim3(kStepThreads), 0, stream, sa);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_tsne_gradient(const float* P, int64_t n, const float* Y, double exaggeration, double* out,
                                 float* grad, void* workspace, void* stream) {
  return dad_tsne_gradient_chunked(P, n, Y, exaggeration, out, grad, 0, workspace, stream);
}

extern "C" int dad_tsne_run(const float* P, int64_t n, float* Y, const dad_tsne_args* args, double* history,
                            double* out, void* ws, void* stream_) {
  if (!P || !Y || !args || !history || !out || !ws) return DAD_E_ARG;
  if (n < 2 || n > DAD_TS_MAX_N) return DAD_E_SHAPE;
  if (args->max_iter < 1 || args->n_iter_without_progress < 0 || !(args->early_exaggeration > 0.0) ||
      !(args->learning_rate > 0.0))
    return DAD_E_ARG;
  PairPlan pl;
  DAD_RET(pair_resolve(n, 0, kMaxChunks, dad_tsne_plan, &pl));
  hipStream_t stream = (hipStream_t)stream_;
  const TsneWs L = tsne_ws_layout(n);
  RunHdr* hdr = ws_ptr<RunHdr>(ws, L.hdr + 64);
  TsneStepArgs sa = {};
  sa.part = ws_ptr<float>(ws, L.part); sa.partd = ws_ptr<double>(ws, L.partd);
  sa.Y = Y; sa.upd = ws_ptr<float>(ws, L.upd); sa.gains = ws_ptr<float>(ws, L.gains);
  sa.hdr = hdr; sa.history = history; sa.out = out;
  sa.n = (int)n; sa.npad = pl.rt * kTile; sa.chunks = pl.chunks;
  sa.max_iter = args->max_iter;
  sa.explore_n = args->max_iter < kExplore ? args->max_iter : kExplore;
  sa.nwp = args->n_iter_without_progress;
  sa.lr = (float)args->learning_rate; sa.early_ex = (float)args->early_exaggeration; sa.ex = 1.0f;
  sa.min_grad_norm = args->min_grad_norm;
  hipLaunchKernelGGL(dad_tsne_init, dim3(1), dim3(kStepThreads), 0, stream, hdr, sa.upd, sa.gains, out, (int)n);
  DAD_TRY(hipGetLastError());
  for (int it = 0; it < args->max_iter; ++it) {
    sa.it = it;
    sa.check = (it + 1) % kCheck == 0;
    sa.compute = sa.check || it == sa.explore_n - 1 || it == args->max_iter - 1;
    DAD_RET(launch_force(P, Y, n, pl, L, ws, sa.compute != 0, &hdr->stop, stream));
    hipLaunchKernelGGL(dad_tsne_step<true>, dim3(1), dim3(kStepThreads), 0, stream, sa);
    DAD_TRY(hipGetLastError());
  }
  return DAD_OK;
}
