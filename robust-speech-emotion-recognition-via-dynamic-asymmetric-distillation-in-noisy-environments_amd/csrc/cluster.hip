// Class separation of a split's embeddings on the device: silhouette and Calinski-Harabasz.
//
// Replaces calculate_cluster_metrics (I/iemocap_plot_tsne.py:390-398): scikit-learn's silhouette_score
// and calinski_harabasz_score on the [n][256] embeddings of a split, with scikit-learn's meaning
// (include/dad.h restates it).  Six launches, no floating-point atomics, every sum in a fixed order:
//
//   dad_pair_prep      (pairwise.hip, 4 groups: the row's class) one workgroup per 64-row tile: the tile's per-class
//                      column sums in double, its class counts and its count of labelled rows with a non-finite
//                      component
//   dad_cluster_stats  one workgroup: dad_pair_reduce (pairwise.h: class sums over the tiles in tile order ->
//                      counts, m, the centroids in double, the labelled rows' mean mu rounded to fp32), then k,
//                      the valid flag and B
//   dad_pair_norms     (pairwise.hip) |x_i - mu|^2 per row, as the diagonal of the pair kernel's own Gram block.
//                      Distances do not change under a shift, and post-ReLU embeddings share a large positive
//                      mean: with every operand centred on mu the identity |a|^2 + |b|^2 - 2 a.b cancels
//                      numbers of the size of the spread, not of the mean (|x|^2 ~ 90 against |x - mu|^2 ~ 3
//                      on the tests' inputs).  Both kernels subtract the same fp32 mu from the same fp32 x.
//   dad_cluster_pair   the n x n pass.  Workgroup (row tile, chunk) owns 64 rows and a contiguous run of
//                      64-column tiles.  Each of its 4 waves holds 32 rows of the row tile in registers as
//                      the A operand of v_mfma_f32_32x32x2_f32 (lane = row, 4 consecutive k per k-block of
//                      8 and lane half) and owns one 32 x 32 quadrant of every 64 x 64 tile; the column
//                      tile's rows are staged through LDS (row stride 260 floats: the 16-byte operand reads
//                      of 8 consecutive rows cover the 32 banks once), with the columns' norms and labels.
//                      The epilogue turns the Gram block into distances, zeroes the diagonal, and adds each
//                      distance to the bin of its column's class, per lane; unlabelled and padding columns
//                      match no bin.  After the last tile the bins cross the 32 lanes of a row by a fixed
//                      xor tree, the two column halves meet in LDS, and the workgroup writes its [64][4]
//                      sums to the workspace.  The distance matrix never exists in memory.
//   dad_cluster_rows   one workgroup per row tile: adds the chunks in chunk order, forms a, b, s per row,
//                      |x_i - mu_c|^2 in double, and the tile's sums of s per class and of W
//   dad_cluster_final  one workgroup: the tiles in tile order -> the result block
//
// Work per call (rt = ceil(n / 64) row tiles): the pair kernel runs 2 * 256 * (64 rt)^2 FLOP on the fp32 matrix
// cores and stages rt * rt column tiles of 64 KB plus rt * chunks row tiles from L2 (the embeddings are 1 KB a
// row); the other launches read the embeddings three more times.  DESIGN.md 6b has the measured figures.
#include <cstdint>

#include "dad_common.h"
#include "pairwise.h"   // the centring prologue, the Gram walk, the bin flush and the chunk plan (shared)

namespace {

constexpr int kTile = DAD_CM_TILE;         // rows and columns of a tile
constexpr int kLd = kGramLd;               // LDS row stride of the column tile, floats
constexpr int kThreads = kGramThreads;
constexpr int kMaxChunks = DAD_CM_MAX_CHUNKS;

static_assert(kTile == 64 && DAD_H == 256 && DAD_C == 4, "the pair kernel's wave / lane mapping");

struct ClusterWs {
  size_t norms, part, csum, cnt, cent, mean, hdr_i, hdr_d, wpart, silpart, bytes;
};

// (a function of n alone: the chunk count a call runs with is at most min(column tiles, kMaxChunks))
ClusterWs cluster_ws_layout(int64_t n) {
  ClusterWs w;
  const size_t rt = (size_t)((n + kTile - 1) / kTile), npad = rt * kTile;
  const size_t maxc = rt < (size_t)kMaxChunks ? rt : (size_t)kMaxChunks;
  size_t off = 0;
  w.norms = off;   off = dad_align(off + sizeof(float) * npad);
  w.part = off;    off = dad_align(off + sizeof(float) * maxc * npad * DAD_C);
  w.csum = off;    off = dad_align(off + sizeof(double) * rt * DAD_C * DAD_H);
  w.cnt = off;     off = dad_align(off + sizeof(int32_t) * rt * (DAD_C + 1));
  w.cent = off;    off = dad_align(off + sizeof(double) * DAD_C * DAD_H);
  w.mean = off;    off = dad_align(off + sizeof(float) * DAD_H);
  w.hdr_i = off;   off = dad_align(off + sizeof(int32_t) * 8);
  w.hdr_d = off;   off = dad_align(off + sizeof(double) * 2);
  w.wpart = off;   off = dad_align(off + sizeof(double) * rt);
  w.silpart = off; off = dad_align(off + sizeof(double) * rt * DAD_C);
  w.bytes = off;
  return w;
}

// hdr_i slots
constexpr int kHN0 = 0, kHM = 4, kHK = 5, kHValid = 6, kHBad = 7;

}  // namespace

__global__ __launch_bounds__(kThreads) void dad_cluster_stats(const double* __restrict__ csum,
                                                              const int32_t* __restrict__ cnt, int rt,
                                                              double* __restrict__ cent, float* __restrict__ mean,
                                                              int32_t* __restrict__ hdr_i,
                                                              double* __restrict__ hdr_d) {
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const PairStats<DAD_C> p = dad_pair_reduce<DAD_C>(csum, cnt, rt, tid, cent);
  const int* nc = p.nc;
  const int m = p.m, k = (nc[0] > 0) + (nc[1] > 0) + (nc[2] > 0) + (nc[3] > 0);
  mean[tid] = p.mean;
  double b = 0.0;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c)
    b += nc[c] > 0 ? (double)nc[c] * ((p.mc[c] - p.mu) * (p.mc[c] - p.mu)) : 0.0;
  red[tid] = b;
  __syncthreads();
  if (tid == 0) {
    double bs = 0.0;
    for (int d = 0; d < kThreads; ++d) bs += red[d];
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) hdr_i[kHN0 + c] = nc[c];
    hdr_i[kHM] = m;
    hdr_i[kHK] = k;
    hdr_i[kHValid] = k >= 2 && k <= m - 1;
    hdr_i[kHBad] = p.bad;
    hdr_d[0] = bs;
  }
}

struct ClusterPairArgs {
  const float* emb;
  const int64_t* labels;
  const float* norms;
  const float* mean;
  float* part;      // [chunks][npad][4]
  int n, npad, ct, per;
};

// (two workgroups per CU, so one stages its next column tile while the other multiplies: 256 registers a lane)
__global__ __launch_bounds__(kThreads, 2) void dad_cluster_pair(ClusterPairArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kLd];
  __shared__ float nj_s[kTile], ni_s[kTile];
  __shared__ int lj_s[kTile];
  const int tid = threadIdx.x;
  const GramLane g = dad_gram_lane(tid);
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y;
  float bins[16][DAD_C];
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) bins[r][c] = 0.0f;

  dad_gram_walk_chunk(
      a.emb, a.norms, a.mean, a.n, i0, chunk, a.per, a.ct, bt, nj_s, ni_s,
      [&](int c, int j) { lj_s[c] = j < a.n ? class_of(a.labels[j]) : -1; },
      [&](int r, int, int jc, int, float d2) {
        const int cj = lj_s[jc];
        const float d = sqrtf(d2);
#pragma unroll
        for (int c = 0; c < DAD_C; ++c) bins[r][c] += cj == c ? d : 0.0f;
      });
  flush_bins<DAD_C>(bins, g, bt, a.part + ((size_t)chunk * a.npad + i0) * DAD_C);
}

struct ClusterRowArgs {
  const float* emb;
  const int64_t* labels;
  const float* part;
  const double* cent;
  const int32_t* hdr_i;
  float* sil;        // [n] or NULL
  double* wpart;     // [rt]
  double* silpart;   // [rt][4]
  int n, npad, chunks;
};

__global__ __launch_bounds__(kThreads) void dad_cluster_rows(ClusterRowArgs a) {
  __shared__ int lab_s[kTile];
  __shared__ double w_s[kTile], s_s[kTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, i0 = kTile * tile, n = a.n;
  if (tid < kTile) {
    const int i = i0 + tid;
    const int c = i < n ? class_of(a.labels[i]) : -1;
    lab_s[tid] = c;
    double s = 0.0;
    if (c >= 0 && a.hdr_i[kHValid]) {
      float sum[DAD_C] = {0.0f, 0.0f, 0.0f, 0.0f};
      dad_chunk_sum4(sum, a.part, a.chunks, a.npad, i);
      double own = 0.0, other = 0.0;
      int nown = 0;
      bool have = false;
#pragma unroll
      for (int k = 0; k < DAD_C; ++k) {
        const int nk = a.hdr_i[kHN0 + k];
        if (k == c) {
          own = (double)sum[k];
          nown = nk;
        } else if (nk > 0) {
          const double mean = (double)sum[k] / (double)nk;
          other = have ? (mean < other ? mean : other) : mean;
          have = true;
        }
      }
      if (nown > 1 && have) {
        const double av = own / (double)(nown - 1);
        const double mx = av > other ? av : other;
        s = mx > 0.0 ? (other - av) / mx : 0.0;
      }
    }
    s_s[tid] = s;
    if (a.sil && i < n) a.sil[i] = (float)s;
  }
  __syncthreads();
  for (int rr = w; rr < kTile; rr += kThreads / 64) {
    const int c = lab_s[rr];         // (uniform in the wave)
    const double ws =
        c >= 0 ? dad_row_compactness(a.emb + (size_t)(i0 + rr) * DAD_H, a.cent + c * DAD_H, lane) : 0.0;
    if (lane == 0) w_s[rr] = ws;
  }
  __syncthreads();
  if (tid < DAD_C) {
    double s = 0.0;
    for (int rr = 0; rr < kTile; ++rr) s += lab_s[rr] == tid ? s_s[rr] : 0.0;
    a.silpart[tile * DAD_C + tid] = s;
  } else if (tid == DAD_C) {
    double s = 0.0;
    for (int rr = 0; rr < kTile; ++rr) s += w_s[rr];
    a.wpart[tile] = s;
  }
}

__global__ __launch_bounds__(64) void dad_cluster_final(const double* __restrict__ wpart,
                                                        const double* __restrict__ silpart,
                                                        const int32_t* __restrict__ hdr_i,
                                                        const double* __restrict__ hdr_d, int rt,
                                                        double* __restrict__ out) {
  __shared__ double v_s[DAD_C + 1];
  const int tid = threadIdx.x;
  if (tid <= DAD_C) {
    double s = 0.0;
    if (tid < DAD_C) for (int t = 0; t < rt; ++t) s += silpart[t * DAD_C + tid];
    else for (int t = 0; t < rt; ++t) s += wpart[t];
    v_s[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    const int m = hdr_i[kHM], k = hdr_i[kHK];
    const bool valid = hdr_i[kHValid] != 0;
    const double W = v_s[DAD_C], B = hdr_d[0];
    const double stot = ((v_s[0] + v_s[1]) + v_s[2]) + v_s[3];
    out[DAD_CM_SILHOUETTE] = valid ? stot / (double)m : 0.0;
    out[DAD_CM_CH] = !valid ? 0.0 : (W == 0.0 ? 1.0 : (B * (double)(m - k)) / (W * ((double)k - 1.0)));
    out[DAD_CM_VALID] = valid ? 1.0 : 0.0;
    out[DAD_CM_M] = (double)m;
    out[DAD_CM_K] = (double)k;
    for (int c = 0; c < DAD_C; ++c) {
      const int nc = hdr_i[kHN0 + c];
      out[DAD_CM_COUNTS + c] = (double)nc;
      out[DAD_CM_SIL_CLASS + c] = valid && nc > 0 ? v_s[c] / (double)nc : 0.0;
    }
    out[DAD_CM_W] = W;
    out[DAD_CM_B] = B;
    out[DAD_CM_NONFINITE] = (double)hdr_i[kHBad];
  }
}

extern "C" int dad_cluster_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  return pair_plan_resident2(n, cus, DAD_CM_MAX_N, kMaxChunks, row_tiles, chunks, tiles_per_chunk);
}

extern "C" size_t dad_cluster_workspace_bytes(int64_t n) {
  if (n < 1 || n > DAD_CM_MAX_N) return 0;
  return cluster_ws_layout(n).bytes;
}

extern "C" int dad_cluster_metrics_chunked(const float* emb, const int64_t* labels, int64_t n, double* out, float* sil,
                                           int chunks, void* ws, void* stream_) {
  if (!emb || !labels || !out || !ws) return DAD_E_ARG;
  if (n < 1 || n > DAD_CM_MAX_N) return DAD_E_SHAPE;
  PairPlan pl;
  DAD_RET(pair_resolve(n, chunks, kMaxChunks, dad_cluster_plan, &pl));
  const int rt = pl.rt;
  hipStream_t stream = (hipStream_t)stream_;
  const ClusterWs L = cluster_ws_layout(n);
  float *norms = ws_ptr<float>(ws, L.norms), *part = ws_ptr<float>(ws, L.part), *mean = ws_ptr<float>(ws, L.mean);
  double *csum = ws_ptr<double>(ws, L.csum), *cent = ws_ptr<double>(ws, L.cent), *hdr_d = ws_ptr<double>(ws, L.hdr_d);
  double *wpart = ws_ptr<double>(ws, L.wpart), *silpart = ws_ptr<double>(ws, L.silpart);
  int32_t *cnt = ws_ptr<int32_t>(ws, L.cnt), *hdr_i = ws_ptr<int32_t>(ws, L.hdr_i);

  const auto stats = [&] {
    hipLaunchKernelGGL(dad_cluster_stats, dim3(1), dim3(kThreads), 0, stream, csum, cnt, rt, cent, mean, hdr_i, hdr_d);
  };
  DAD_RET((pair_centre<DAD_C, false>(emb, PairClassGroup{labels}, nullptr, n, rt, csum, cnt, nullptr, mean, norms,
                                     stream, stats)));
  ClusterPairArgs pa;
  pa.emb = emb; pa.labels = labels; pa.norms = norms; pa.mean = mean; pa.part = part;
  pa.n = (int)n; pa.npad = rt * kTile; pa.ct = rt; pa.per = pl.per;
  hipLaunchKernelGGL(dad_cluster_pair, dim3(rt, pl.chunks), dim3(kThreads), 0, stream, pa);
  DAD_TRY(hipGetLastError());
  ClusterRowArgs ra;
  ra.emb = emb; ra.labels = labels; ra.part = part; ra.cent = cent; ra.hdr_i = hdr_i; ra.sil = sil;
  ra.wpart = wpart; ra.silpart = silpart; ra.n = (int)n; ra.npad = rt * kTile; ra.chunks = pl.chunks;
  hipLaunchKernelGGL(dad_cluster_rows, dim3(rt), dim3(kThreads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_cluster_final, dim3(1), dim3(64), 0, stream, wpart, silpart, hdr_i, hdr_d, rt, out);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_cluster_metrics(const float* emb, const int64_t* labels, int64_t n, double* out, float* sil,
                                   void* workspace, void* stream) {
  return dad_cluster_metrics_chunked(emb, labels, n, out, sil, 0, workspace, stream);
}
