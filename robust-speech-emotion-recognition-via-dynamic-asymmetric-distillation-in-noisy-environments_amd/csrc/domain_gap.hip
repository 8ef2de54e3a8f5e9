// The clean-noisy domain gap of two splits' embeddings on the device: ECDALoss (I/utils.py:510-652) on whole splits.
//
// The attention-weighted multi-bandwidth Gaussian MMD per class and over all rows, the compactness of each class's
// noisy rows, the repulsion of the noisy centroids and their weighted sum, with the reference's meaning (include/dad.h
// restates it).  _gaussian_kernel expands [m][m][256] temporaries; here the distance matrix never exists in memory.
// Nine launches, no floating-point atomics, every sum in a fixed order.  A row's group is 2 * class + domain, or -1
// for a row that takes no part (label outside [0, 4)); such rows and the padding behind row n are left out by
// selection everywhere, never by a multiplication, so a NaN in them reaches no sum.
//
//   dad_pair_prep      (pairwise.hip, 8 groups, with weights) one workgroup per 64-row tile: the tile's per-group
//                      column sums in double, its group counts and weight sums, and its count of participating rows
//                      with a non-finite component
//   dad_dg_stats       one workgroup: dad_pair_reduce (pairwise.h: the tiles in tile order -> counts, the centroids in
//                      double, the participating rows' mean mu rounded to fp32), then the weight sums, the centroid
//                      shifts and the repulsion
//   dad_pair_norms     (pairwise.hip) |x_i - mu|^2 as the diagonal of the walk's own Gram block
//   dad_dg_pass1       the first n x n walk (pairwise.h): per row, the sums of d2 over the participating columns and
//                      over the columns of the row's own class, per column chunk
//   dad_dg_rows1       one workgroup per row tile: adds the chunks in chunk order and the rows in row order ->
//                      the tile's sum of d2 over each class's pairs and over all pairs
//   dad_dg_bandwidth   one workgroup: the tiles in tile order -> the bandwidth of each class and of the global set
//                      in double, and the fp32 coefficients -log2(e) / (bw 2^b + 1e-8), b = 0 .. 4, so that an
//                      exponential is one multiply and one v_exp_f32
//   dad_dg_pass2       the second walk.  Each distance gets 5 exponentials for the global kernel and 5 more when
//                      row and column share a class; per row and per column domain it adds K_global and
//                      w_j K_class.  The global coefficients sit in scalar registers, the classes' table in LDS, and
//                      nothing of a column lives across the next tile's staging: 16 x 4 bins per lane, as
//                      dad_cluster_pair.
//   dad_dg_rows2       one workgroup per row tile: adds the chunks in chunk order, applies w_i, bins by (class, row
//                      domain, column domain) in double, and adds |x_i - centroid|^2 of the noisy rows
//   dad_dg_final       one workgroup: the tiles in tile order -> the result block
//
// Work per call (rt = ceil(n / 64) row tiles): two walks of 2 * 256 * (64 rt)^2 FLOP each on the fp32 matrix cores,
// up to 10 exponentials per pair in the second.  DESIGN.md 6b has the figures.
#include <cstdint>

#include "dad_common.h"
#include "pairwise.h"

namespace {

constexpr int kTile = kGramTile;
constexpr int kThreads = kGramThreads;
constexpr int kMaxChunks = DAD_DG_MAX_CHUNKS;
constexpr int kG = 2 * DAD_C;              // groups: 2 * class + domain
constexpr int kNB = 5;                     // kernel_num; kernel_mul = 2 (the train step's tail fixes both)
constexpr int kSets = DAD_C + 1;           // the classes' sets and the global one
constexpr int kBins = 24;                  // rows2: class [4][2][2], global [2][2], compactness [4]

static_assert(kTile == 64 && DAD_H == 256 && DAD_C == 4 && kTile == DAD_DG_TILE, "the walk's wave / lane mapping");

struct GapWs {
  size_t norms, part, csum, cnt, wsum, cent, mean, hdr_i, hdr_d, dsum, bw, coef, bins, bytes;
};

// (a function of n alone: the chunk count a call runs with is at most min(column tiles, kMaxChunks))
GapWs gap_ws_layout(int64_t n) {
  GapWs w;
  const size_t rt = (size_t)((n + kTile - 1) / kTile), npad = rt * kTile;
  const size_t maxc = rt < (size_t)kMaxChunks ? rt : (size_t)kMaxChunks;
  size_t off = 0;
  w.norms = off; off = dad_align(off + sizeof(float) * npad);
  w.part = off;  off = dad_align(off + sizeof(float) * maxc * npad * 4);     // pass 1 [..][2], then pass 2 [..][4]
  w.csum = off;  off = dad_align(off + sizeof(double) * rt * kG * DAD_H);
  w.cnt = off;   off = dad_align(off + sizeof(int32_t) * rt * (kG + 1));
  w.wsum = off;  off = dad_align(off + sizeof(double) * rt * kG);
  w.cent = off;  off = dad_align(off + sizeof(double) * kG * DAD_H);
  w.mean = off;  off = dad_align(off + sizeof(float) * DAD_H);
  w.hdr_i = off; off = dad_align(off + sizeof(int32_t) * 16);
  w.hdr_d = off; off = dad_align(off + sizeof(double) * 16);
  w.dsum = off;  off = dad_align(off + sizeof(double) * rt * kSets);
  w.bw = off;    off = dad_align(off + sizeof(double) * kSets);
  w.coef = off;  off = dad_align(off + sizeof(float) * kSets * kNB);
  w.bins = off;  off = dad_align(off + sizeof(double) * rt * kBins);
  w.bytes = off;
  return w;
}

// hdr_i: [0, 8) group counts, 8 bad rows.  hdr_d: [0, 8) group weight sums, [8, 12) centroid shifts, 12 repulsion
constexpr int kHBad = 8, kHShift = 8, kHRep = 12;

// 2 * class + domain of row i, -1 for a row that takes no part
__device__ __forceinline__ int group_of(const int64_t* __restrict__ labels, const uint8_t* __restrict__ domain, int i,
                                        int n) {
  return i < n ? PairDomainGroup{labels, domain}(i) : -1;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void dad_dg_stats(const double* __restrict__ csum,
                                                         const int32_t* __restrict__ cnt,
                                                         const double* __restrict__ wsum, int rt,
                                                         double* __restrict__ cent, float* __restrict__ mean,
                                                         int32_t* __restrict__ hdr_i, double* __restrict__ hdr_d) {
  constexpr int kRed = DAD_C + DAD_C * (DAD_C - 1) / 2;     // 4 shifts, 6 centroid pairs
  __shared__ double red[kRed][kThreads];
  const int tid = threadIdx.x;
  const PairStats<kG> st = dad_pair_reduce<kG>(csum, cnt, rt, tid, cent);
  const double* mc = st.mc;
  const int* nc = st.nc;
  mean[tid] = st.mean;
  int q = DAD_C;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    const double d = mc[2 * c] - mc[2 * c + 1];
    red[c][tid] = d * d;
#pragma unroll
    for (int e = c + 1; e < DAD_C; ++e) {
      const double p = mc[2 * c + 1] - mc[2 * e + 1];
      red[q++][tid] = p * p;
    }
  }
  __syncthreads();
  if (tid < kRed) {
    double v = 0.0;
    for (int d = 0; d < kThreads; ++d) v += red[tid][d];
    red[tid][0] = sqrt(v);
  }
  __syncthreads();
  if (tid < kG) {
    double v = 0.0;
    for (int t = 0; t < rt; ++t) v += wsum[t * kG + tid];
    hdr_d[tid] = v;
  } else if (tid == kG) {
#pragma unroll
    for (int k = 0; k < kG; ++k) hdr_i[k] = nc[k];
    hdr_i[kHBad] = st.bad;
    // shifts; the repulsion: minus the mean distance of the noisy centroids of the classes with a noisy row
    double rep = 0.0;
    int pairs = 0, p = DAD_C;
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) {
      hdr_d[kHShift + c] = nc[2 * c] > 0 && nc[2 * c + 1] > 0 ? red[c][0] : 0.0;
#pragma unroll
      for (int e = c + 1; e < DAD_C; ++e, ++p)
        if (nc[2 * c + 1] > 0 && nc[2 * e + 1] > 0) {
          rep += red[p][0];
          pairs += 1;
        }
    }
    hdr_d[kHRep] = pairs > 0 ? -(rep / (double)pairs) : 0.0;
  }
}

struct GapPassArgs {
  const float* emb;
  const int64_t* labels;
  const uint8_t* domain;
  const float* weights;
  const float* norms;
  const float* mean;
  const float* coef;   // [5 sets][5] (pass 2)
  float* part;         // [chunks][npad][2] (pass 1), [chunks][npad][4] (pass 2)
  int n, npad, ct, per;
};

__global__ __launch_bounds__(kThreads, 2) void dad_dg_pass1(GapPassArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ float nj_s[kTile], ni_s[kTile];
  __shared__ int cj_s[kTile], ci_s[kTile];
  const int tid = threadIdx.x;
  const GramLane g = dad_gram_lane(tid);
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y;
  if (tid < kTile) {
    const int gi = group_of(a.labels, a.domain, i0 + tid, a.n);
    ci_s[tid] = gi < 0 ? -2 : gi >> 1;           // (-2: matches no column, not even one that takes no part)
  }
  float bins[16][2];
#pragma unroll
  for (int r = 0; r < 16; ++r) bins[r][0] = bins[r][1] = 0.0f;
  dad_gram_walk_chunk(
      a.emb, a.norms, a.mean, a.n, i0, chunk, a.per, a.ct, bt, nj_s, ni_s,
      [&](int c, int j) {
        const int gj = group_of(a.labels, a.domain, j, a.n);
        cj_s[c] = gj < 0 ? -1 : gj >> 1;
      },
      [&](int r, int ig, int jc, int, float d2) {
        const int cj = cj_s[jc], ci = ci_s[ig - i0];
        bins[r][0] += cj >= 0 ? d2 : 0.0f;
        bins[r][1] += cj == ci ? d2 : 0.0f;
      });
  flush_bins<2>(bins, g, bt, a.part + ((size_t)chunk * a.npad + i0) * 2);
}

// per tile: sum over its rows of a class of the row's own-class d2 sum -> dsum[tile][class]; of every participating
// row's d2 sum over the participating columns -> dsum[tile][4]
__global__ __launch_bounds__(kTile) void dad_dg_rows1(const int64_t* __restrict__ labels,
                                                      const uint8_t* __restrict__ domain,
                                                      const float* __restrict__ part, int n, int npad, int chunks,
                                                      double* __restrict__ dsum) {
  __shared__ int c_s[kTile];
  __shared__ double v_s[kTile][2];
  const int tid = threadIdx.x, tile = blockIdx.x, i = kTile * tile + tid;
  const int gi = group_of(labels, domain, i, n);
  float all = 0.0f, own = 0.0f;
  if (gi >= 0)
    for (int q = 0; q < chunks; ++q) {
      const float* p = part + ((size_t)q * npad + i) * 2;
      all += p[0];
      own += p[1];
    }
  c_s[tid] = gi < 0 ? -1 : gi >> 1;
  v_s[tid][0] = (double)all;
  v_s[tid][1] = (double)own;
  __syncthreads();
  if (tid < kSets) {
    double s = 0.0;
    for (int rr = 0; rr < kTile; ++rr)
      if (tid < DAD_C ? c_s[rr] == tid : c_s[rr] >= 0) s += v_s[rr][tid < DAD_C ? 1 : 0];
    dsum[tile * kSets + tid] = s;
  }
}

__global__ __launch_bounds__(64) void dad_dg_bandwidth(const double* __restrict__ dsum,
                                                       const int32_t* __restrict__ hdr_i, int rt,
                                                       double* __restrict__ bw, float* __restrict__ coef) {
  const int tid = threadIdx.x;
  if (tid >= kSets) return;
  double s = 0.0;
  for (int t = 0; t < rt; ++t) s += dsum[t * kSets + tid];
  double m = 0.0;
  for (int k = 0; k < kG; ++k)
    if (tid == DAD_C || (k >> 1) == tid) m += (double)hdr_i[k];
  // bandwidth = sum(L2) / (m^2 - m) / kernel_mul^(kernel_num / 2)
  const double b0 = m > 1.0 ? s / (m * m - m) / 4.0 : 0.0;
  bw[tid] = b0;
  double mul = 1.0;
  for (int b = 0; b < kNB; ++b, mul *= 2.0) coef[tid * kNB + b] = (float)(-1.4426950408889634 / (b0 * mul + 1e-8));
}

// (two workgroups per CU as dad_cluster_pair: 128 registers of A operand, 16 x 4 bins, 256 a lane)
__global__ __launch_bounds__(kThreads, 2) void dad_dg_pass2(GapPassArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ float nj_s[kTile], ni_s[kTile], wj_s[kTile];
  __shared__ int gj_s[kTile], ci_s[kTile];
  const int tid = threadIdx.x;
  const GramLane g = dad_gram_lane(tid);
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y;
  if (tid < kTile) {
    const int gi = group_of(a.labels, a.domain, i0 + tid, a.n);
    ci_s[tid] = gi < 0 ? -2 : gi >> 1;
  }
  __shared__ float coef_s[kSets * kNB];
  if (tid < kSets * kNB) coef_s[tid] = a.coef[tid];
  float cg[kNB];        // the global set's coefficients (uniform: scalar registers)
#pragma unroll
  for (int b = 0; b < kNB; ++b) cg[b] = a.coef[DAD_C * kNB + b];
  float bins[16][4];    // K_global by column domain, w_j K_class by column domain
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) bins[r][c] = 0.0f;

  dad_gram_walk_chunk(
      a.emb, a.norms, a.mean, a.n, i0, chunk, a.per, a.ct, bt, nj_s, ni_s,
      [&](int c, int j) {
        const int gj = group_of(a.labels, a.domain, j, a.n);
        gj_s[c] = gj;
        wj_s[c] = gj >= 0 ? (a.weights ? a.weights[j] : 1.0f) : 0.0f;
      },
      [&](int r, int ig, int jc, int, float d2) {
        // (the lane's column is the same for its 16 entries of a tile: these reads happen once per tile, and
        // nothing of the column lives across the next tile's staging)
        const int gj = gj_s[jc], cj = gj < 0 ? -1 : gj >> 1;
        const bool in0 = gj >= 0 && (gj & 1) == 0, in1 = gj >= 0 && (gj & 1) == 1;
        float kg = 0.0f;
#pragma unroll
        for (int b = 0; b < kNB; ++b) kg += __builtin_amdgcn_exp2f(d2 * cg[b]);
        float kc = 0.0f;
        if (ci_s[ig - i0] == cj) {
          const float* ck = &coef_s[cj * kNB];       // (cj >= 0 here)
#pragma unroll
          for (int b = 0; b < kNB; ++b) kc += __builtin_amdgcn_exp2f(d2 * ck[b]);
          kc *= wj_s[jc];
        }
        bins[r][0] += in0 ? kg : 0.0f;
        bins[r][1] += in1 ? kg : 0.0f;
        bins[r][2] += in0 ? kc : 0.0f;
        bins[r][3] += in1 ? kc : 0.0f;
      });
  flush_bins<4>(bins, g, bt, a.part + ((size_t)chunk * a.npad + i0) * 4);
}

struct GapRowArgs {
  const float* emb;
  const int64_t* labels;
  const uint8_t* domain;
  const float* weights;
  const float* part;
  const double* cent;
  double* bins;        // [rt][24]
  int n, npad, chunks;
};

__global__ __launch_bounds__(kThreads) void dad_dg_rows2(GapRowArgs a) {
  __shared__ int g_s[kTile];
  __shared__ double v_s[kTile][4], w_s[kTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, i0 = kTile * tile, n = a.n;
  if (tid < kTile) {
    const int i = i0 + tid;
    const int gi = group_of(a.labels, a.domain, i, n);
    g_s[tid] = gi;
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double wi = 0.0;
    if (gi >= 0) {
      dad_chunk_sum4(sum, a.part, a.chunks, a.npad, i);
      wi = a.weights ? (double)a.weights[i] : 1.0;
    }
    v_s[tid][0] = (double)sum[0];
    v_s[tid][1] = (double)sum[1];
    v_s[tid][2] = wi * (double)sum[2];
    v_s[tid][3] = wi * (double)sum[3];
  }
  __syncthreads();
  for (int rr = w; rr < kTile; rr += kThreads / 64) {
    const int gi = g_s[rr];          // (uniform in the wave)
    // a noisy row: |x - its class's noisy centroid|^2
    const double ws = gi >= 0 && (gi & 1)
                          ? dad_row_compactness(a.emb + (size_t)(i0 + rr) * DAD_H, a.cent + gi * DAD_H, lane) : 0.0;
    if (lane == 0) w_s[rr] = ws;
  }
  __syncthreads();
  if (tid < kBins) {
    double s = 0.0;
    if (tid < 16) {                  // class tid >> 2, row domain (tid >> 1) & 1, column domain tid & 1
      for (int rr = 0; rr < kTile; ++rr) s += g_s[rr] == (tid >> 1) ? v_s[rr][2 + (tid & 1)] : 0.0;
    } else if (tid < 20) {           // global: row domain (tid >> 1) & 1, column domain tid & 1
      for (int rr = 0; rr < kTile; ++rr)
        s += g_s[rr] >= 0 && (g_s[rr] & 1) == ((tid >> 1) & 1) ? v_s[rr][tid & 1] : 0.0;
    } else {
      for (int rr = 0; rr < kTile; ++rr) s += g_s[rr] == 2 * (tid - 20) + 1 ? w_s[rr] : 0.0;
    }
    a.bins[tile * kBins + tid] = s;
  }
}

__global__ __launch_bounds__(64) void dad_dg_final(const double* __restrict__ bins, const int32_t* __restrict__ hdr_i,
                                                   const double* __restrict__ hdr_d, const double* __restrict__ bw,
                                                   int rt, dad_domain_gap_args args, double* __restrict__ out) {
  __shared__ double v_s[kBins];
  const int tid = threadIdx.x;
  if (tid < kBins) {
    double s = 0.0;
    for (int t = 0; t < rt; ++t) s += bins[t * kBins + tid];
    v_s[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int k = 0; k < DAD_DG_SLOTS; ++k) out[k] = 0.0;
  int ns = 0, nt = 0;
  for (int c = 0; c < DAD_C; ++c) {
    ns += hdr_i[2 * c];
    nt += hdr_i[2 * c + 1];
  }
  const double cw_mean = ((((double)args.class_weights[0] + (double)args.class_weights[1]) +
                           (double)args.class_weights[2]) + (double)args.class_weights[3]) / 4.0;
  const double rep = hdr_d[kHRep];
  bool any = false;
  double loss = 0.0, mmd_sum = 0.0;
  int open = 0;
  for (int c = 0; c < DAD_C; ++c) {
    const int nsc = hdr_i[2 * c], ntc = hdr_i[2 * c + 1];
    const double wsc = hdr_d[2 * c], wtc = hdr_d[2 * c + 1];
    const bool gate = nsc >= 2 && ntc >= 2;
    const double att = exp(args.lambda * (cw_mean - (double)args.class_weights[c]));
    out[DAD_DG_C_N_SRC + c] = (double)nsc;
    out[DAD_DG_C_N_TGT + c] = (double)ntc;
    out[DAD_DG_C_W_TGT + c] = wtc;
    out[DAD_DG_C_ATTENTION + c] = att;
    if (!gate) continue;
    const double ss = v_s[4 * c + 0] / (wsc * wsc + 1e-8);
    const double tt = v_s[4 * c + 3] / (wtc * wtc + 1e-8);
    const double st = v_s[4 * c + 1] / (wsc * wtc + 1e-8);
    const double mmd = (ss + tt) - 2.0 * st;
    const double comp = v_s[20 + c] / (double)ntc;
    out[DAD_DG_C_GATE + c] = 1.0;
    out[DAD_DG_C_BANDWIDTH + c] = bw[c];
    out[DAD_DG_C_SS + c] = ss;
    out[DAD_DG_C_TT + c] = tt;
    out[DAD_DG_C_ST + c] = st;
    out[DAD_DG_C_MMD + c] = mmd;
    out[DAD_DG_C_COMPACTNESS + c] = comp;
    out[DAD_DG_C_SHIFT + c] = hdr_d[kHShift + c];
    loss += att * ((mmd + args.gamma * comp) + args.delta * rep);
    mmd_sum += mmd;
    open += 1;
    any = true;
  }
  if (ns >= 2 && nt >= 2) {
    const double s = (double)ns, t = (double)nt;
    const double ss = v_s[16] / (s * s + 1e-8), tt = v_s[19] / (t * t + 1e-8), st = v_s[17] / (s * t + 1e-8);
    out[DAD_DG_G_GATE] = 1.0;
    out[DAD_DG_G_BANDWIDTH] = bw[DAD_C];
    out[DAD_DG_G_SS] = ss;
    out[DAD_DG_G_TT] = tt;
    out[DAD_DG_G_ST] = st;
    out[DAD_DG_G_MMD] = (ss + tt) - 2.0 * st;
    any = true;
  }
  out[DAD_DG_VALID] = any ? 1.0 : 0.0;
  out[DAD_DG_N_SRC] = (double)ns;
  out[DAD_DG_N_TGT] = (double)nt;
  out[DAD_DG_NONFINITE] = (double)hdr_i[kHBad];
  out[DAD_DG_REPULSION] = rep;
  out[DAD_DG_ECDA_LOSS] = loss;
  out[DAD_DG_MMD_CLASS_MEAN] = open > 0 ? mmd_sum / (double)open : 0.0;
}

extern "C" int dad_domain_gap_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  return pair_plan_resident2(n, cus, DAD_DG_MAX_N, kMaxChunks, row_tiles, chunks, tiles_per_chunk);
}

extern "C" size_t dad_domain_gap_workspace_bytes(int64_t n) {
  if (n < 1 || n > DAD_DG_MAX_N) return 0;
  return gap_ws_layout(n).bytes;
}

extern "C" int dad_domain_gap_chunked(const float* emb, const int64_t* labels, const uint8_t* domain,
                                      const float* weights, int64_t n, const dad_domain_gap_args* args, double* out,
                                      int chunks, void* ws, void* stream_) {
  if (!emb || !labels || !domain || !args || !out || !ws) return DAD_E_ARG;
  if (n < 1 || n > DAD_DG_MAX_N) return DAD_E_SHAPE;
  PairPlan pl;
  DAD_RET(pair_resolve(n, chunks, kMaxChunks, dad_domain_gap_plan, &pl));
  const int rt = pl.rt;
  hipStream_t stream = (hipStream_t)stream_;
  const GapWs L = gap_ws_layout(n);
  float *norms = ws_ptr<float>(ws, L.norms), *part = ws_ptr<float>(ws, L.part), *mean = ws_ptr<float>(ws, L.mean);
  float* coef = ws_ptr<float>(ws, L.coef);
  double *csum = ws_ptr<double>(ws, L.csum), *wsum = ws_ptr<double>(ws, L.wsum), *cent = ws_ptr<double>(ws, L.cent);
  double *hdr_d = ws_ptr<double>(ws, L.hdr_d), *dsum = ws_ptr<double>(ws, L.dsum), *bw = ws_ptr<double>(ws, L.bw);
  double* bins = ws_ptr<double>(ws, L.bins);
  int32_t *cnt = ws_ptr<int32_t>(ws, L.cnt), *hdr_i = ws_ptr<int32_t>(ws, L.hdr_i);

  const auto stats = [&] {
    hipLaunchKernelGGL(dad_dg_stats, dim3(1), dim3(kThreads), 0, stream, csum, cnt, wsum, rt, cent, mean, hdr_i, hdr_d);
  };
  DAD_RET((pair_centre<kG, true>(emb, PairDomainGroup{labels, domain}, weights, n, rt, csum, cnt, wsum, mean, norms,
                                 stream, stats)));
  GapPassArgs pa;
  pa.emb = emb; pa.labels = labels; pa.domain = domain; pa.weights = weights; pa.norms = norms; pa.mean = mean;
  pa.coef = coef; pa.part = part; pa.n = (int)n; pa.npad = rt * kTile; pa.ct = rt; pa.per = pl.per;
  hipLaunchKernelGGL(dad_dg_pass1, dim3(rt, pl.chunks), dim3(kThreads), 0, stream, pa);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_dg_rows1, dim3(rt), dim3(kTile), 0, stream, labels, domain, part, (int)n, rt * kTile,
                     pl.chunks, dsum);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_dg_bandwidth, dim3(1), dim3(64), 0, stream, dsum, hdr_i, rt, bw, coef);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_dg_pass2, dim3(rt, pl.chunks), dim3(kThreads), 0, stream, pa);
  DAD_TRY(hipGetLastError());
  GapRowArgs ra;
  ra.emb = emb; ra.labels = labels; ra.domain = domain; ra.weights = weights; ra.part = part; ra.cent = cent;
  ra.bins = bins; ra.n = (int)n; ra.npad = rt * kTile; ra.chunks = pl.chunks;
  hipLaunchKernelGGL(dad_dg_rows2, dim3(rt), dim3(kThreads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_dg_final, dim3(1), dim3(64), 0, stream, bins, hdr_i, hdr_d, bw, rt, *args, out);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_domain_gap(const float* emb, const int64_t* labels, const uint8_t* domain, const float* weights,
                              int64_t n, const dad_domain_gap_args* args, double* out, void* workspace, void* stream) {
  return dad_domain_gap_chunked(emb, labels, domain, weights, n, args, out, 0, workspace, stream);
}
