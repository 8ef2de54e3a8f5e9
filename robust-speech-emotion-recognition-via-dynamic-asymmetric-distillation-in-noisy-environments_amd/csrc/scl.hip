// The supervised-contrastive term of the train loss and its gradient on the device.
//
// SupCon (Khosla et al. 2020, "L_out", no base-temperature factor) as include/dad.h states it: over the member rows A
// (flagged, class in [0, 4), |e| > 1e-12), z = e / |e|, s_ia = z_i . z_a,
//   l_i = -(1 / |P(i)|) sum_{p in P(i)} [ s_ip / tau - log sum_{a in A, a != i} exp(s_ia / tau) ],   L = mean over the
// V anchors with a positive.  The gradient is the closed form  G = H + H^T,  H_ia = (v_i p_ia - c_i [a in P(i)]) /
// (V tau),  gz = G Z,  dL/de_i = (gz_i - z_i (z_i . gz_i)) / |e_i|.  Four launches, ordered by the stream alone; no
// floating-point atomics, every sum in a fixed order:
//
//   dad_scl_prep    one workgroup per 64-row tile: selects the members, normalises them (norm in double) into Z
//                   [npad][256] -- zero rows for everything outside A, so a non-member's values are never an operand --
//                   with each row's class (-1 outside A), 1 / |e|, and the tile's class counts
//   dad_scl_pass1   the n x n pass over the Gram block Z Z^T on the fp32 matrix cores.  Workgroup (row tile, chunk),
//                   the column tile staged in LDS as pairwise.h lays it out (a zero "mean": its d2 would be 2 - 2 s).
//                   The MFMA operands are exchanged against dad_gram_block, so a lane holds 16 columns of ONE row:
//                   the row's running maximum, its sum of exp(s / tau - max) and its positives' sum of s / tau stay in
//                   the lane, and meet the other lane half by one shuffle and the other column half in LDS
//   dad_scl_pass2   the same walk; forms G tile by tile from the rows' and the columns' log-sum-exp (the chunks of
//                   pass one folded in chunk order), hands the tile to LDS and accumulates G Z with MFMA, contracting
//                   over the column tile's rows already staged there.  Wave (rh, ch) owns rows 32 rh.. and output
//                   columns 128 ch.. of the row tile, so no sum crosses waves
//   dad_scl_final   one workgroup per row tile: the chunks of G Z in chunk order, the backward of the normalisation,
//                   the gradient's destination (SclDst); workgroup 0 also sums the anchors' losses in row order
#include <cstdint>

#include "dad_common.h"
#include "pairwise.h"
#include "scl.h"

namespace {

constexpr int kTile = kGramTile;
constexpr int kThreads = kGramThreads;
constexpr int kGsLd = kTile + 32;          // LDS row stride of the G tile: the two lane halves read disjoint banks
constexpr float kNegInf = -__builtin_inff();

static_assert(kTile == 64 && DAD_H == 256 && DAD_C == 4, "the pass kernels' wave / lane mapping");
static_assert(DAD_SCL_MAX_N >= 2 * DAD_MAX_BATCH, "the step's largest batch is one call");

struct SclWs {
  size_t z, cls, invn, zero, cnt, part1, part2, bytes;
};

// (a function of n alone: a call runs with at most min(row tiles, DAD_SCL_MAX_CHUNKS) chunks)
SclWs scl_ws_layout(int64_t n) {
  SclWs w;
  const size_t rt = (size_t)((n + kTile - 1) / kTile), npad = rt * kTile;
  const size_t maxc = rt < (size_t)DAD_SCL_MAX_CHUNKS ? rt : (size_t)DAD_SCL_MAX_CHUNKS;
  size_t off = 0;
  w.z = off;      off = dad_align(off + sizeof(float) * npad * DAD_H);
  w.cls = off;    off = dad_align(off + sizeof(int32_t) * npad);
  w.invn = off;   off = dad_align(off + sizeof(float) * npad);
  w.zero = off;   off = dad_align(off + sizeof(float) * DAD_H);
  w.cnt = off;    off = dad_align(off + sizeof(int32_t) * rt * 8);
  w.part1 = off;  off = dad_align(off + sizeof(float) * maxc * npad * 4);
  w.part2 = off;  off = dad_align(off + sizeof(float) * maxc * npad * DAD_H);
  w.bytes = off;
  return w;
}

struct SclArgs {
  const float* z;        // [npad][256] unit member rows, zeros elsewhere
  const int32_t* cls;    // [npad] class of a member row, -1 elsewhere
  const float* invn;     // [npad] 1 / |e|
  const float* zero;     // [256] zeros: pairwise.h's "mean"
  const int32_t* cnt;    // [rt][8]: class counts [4], flagged rows with a non-finite component
  float* part1;          // [chunks][npad][4]: running maximum of s / tau, sum of exp, positives' sum of s / tau
  float* part2;          // [chunks][npad][256]: the chunk's share of (H + H^T) Z, before the 1 / (V tau)
  int n, npad, rt, per, chunks;
  float inv_tau;
};

__device__ __forceinline__ float scl_exp(float x) { return __expf(x); }

// a row's statistics over a set of columns, and the union of two disjoint sets
struct RowStat {
  float m, l, ps;
};
__device__ __forceinline__ RowStat scl_join(const RowStat& a, const RowStat& b) {
  RowStat r;
  r.m = fmaxf(a.m, b.m);
  r.l = r.m > kNegInf ? a.l * scl_exp(a.m - r.m) + b.l * scl_exp(b.m - r.m) : 0.0f;
  r.ps = a.ps + b.ps;
  return r;
}
// row i over all columns: pass one's chunks in chunk order
__device__ __forceinline__ RowStat scl_row_stat(const float* __restrict__ part1, int chunks, int npad, int i) {
  RowStat s{kNegInf, 0.0f, 0.0f};
  for (int q = 0; q < chunks; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part1 + ((size_t)q * npad + i) * 4);
    s = q == 0 ? RowStat{v[0], v[1], v[2]} : scl_join(s, RowStat{v[0], v[1], v[2]});
  }
  return s;
}
__device__ __forceinline__ float scl_lse(const RowStat& s) { return s.l > 0.0f ? s.m + logf(s.l) : kNegInf; }

// class counts over the tiles in tile order; slot 4: the non-finite count
__device__ __forceinline__ int scl_count(const int32_t* __restrict__ cnt, int rt, int slot) {
  int v = 0;
  for (int t = 0; t < rt; ++t) v += cnt[t * 8 + slot];
  return v;
}

// dad_gram_block with the operands exchanged: acc[r] = z_col . z_row with col = dad_acc_row(r, kh) of the 32 staged
// rows from jc0 on and row = the lane's own (l32), so a lane's 16 entries lie in one row of the Gram block
__device__ __forceinline__ f32x16 scl_gram_block(const f32x4 (&av)[DAD_H / 8], const float* __restrict__ bt, int jc0,
                                                 int l32, int kh) {
  const float* rb = &bt[(jc0 + l32) * kGramLd + 4 * kh];
  f32x16 acc = f32x16{};
#pragma unroll
  for (int q = 0; q < DAD_H / 8; ++q) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(rb + 8 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[e], av[q][e], acc, 0, 0, 0);
  }
  return acc;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void dad_scl_prep(SclSrc s, float* __restrict__ z, int32_t* __restrict__ cls,
                                                         float* __restrict__ invn, float* __restrict__ zero,
                                                         int32_t* __restrict__ cnt) {
  __shared__ int cls_s[kTile], bad_s[kTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, i0 = kTile * tile, n = s.na + s.nb;
  if (tile == 0) zero[tid] = 0.0f;
  for (int rr = w; rr < kTile; rr += kThreads / 64) {
    const int i = i0 + rr;             // (uniform in the wave)
    const float* row = nullptr;
    int c = -1;
    if (i < s.na) {
      const long lab = s.lab_a[i];
      if ((s.mem_a == nullptr || s.mem_a[i] != 0) && lab >= 0 && lab < DAD_C) c = (int)lab;
      row = s.emb_a + (size_t)i * DAD_H;
    } else if (i < n) {
      const float pred = s.pred_b[i - s.na];
      if (s.mask_b[i - s.na] != 0.0f && pred >= 0.0f && pred < (float)DAD_C) c = (int)pred;
      row = s.emb_b + (size_t)(i - s.na) * DAD_H;
    }
    f32x4 zv = f32x4{};
    float inv = 0.0f;
    bool bad = false;
    if (c >= 0) {                      // (a row that is not flagged is not read: its NaNs stay out)
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * lane);
      bad = __ballot(nonfinite(v[0]) | nonfinite(v[1]) | nonfinite(v[2]) | nonfinite(v[3])) != 0ull;
      double p = 0.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) p += (double)v[e] * (double)v[e];
      const double norm = sqrt(dad_wave_sum_d(p));
      if (norm > 1e-12) {              // (NaN: not a member)
#pragma unroll
        for (int e = 0; e < 4; ++e) zv[e] = (float)((double)v[e] / norm);
        inv = (float)(1.0 / norm);
      } else {
        c = -1;
      }
    }
    *reinterpret_cast<f32x4*>(z + (size_t)i * DAD_H + 4 * lane) = zv;   // (npad rows: padding rows get zeros)
    if (lane == 0) {
      cls[i] = c;
      invn[i] = inv;
      cls_s[rr] = c;
      bad_s[rr] = bad;
    }
  }
  __syncthreads();
  if (tid < 8) {
    int v = 0;
    if (tid < DAD_C) for (int rr = 0; rr < kTile; ++rr) v += cls_s[rr] == tid;
    else if (tid == 4) for (int rr = 0; rr < kTile; ++rr) v += bad_s[rr];
    cnt[tile * 8 + tid] = v;
  }
}

__global__ __launch_bounds__(kThreads) void dad_scl_pass1(SclArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ int cls_s[kTile];
  __shared__ __attribute__((aligned(16))) float red[2][kTile][4];
  const int tid = threadIdx.x;
  const GramLane g = dad_gram_lane(tid);
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y;
  const int il = 32 * g.rh + g.l32, ig = i0 + il;
  f32x4 av[DAD_H / 8];
  dad_gram_load_a(av, a.z, a.zero, ig, a.npad, g.kh);
  const f32x4 mu4 = *reinterpret_cast<const f32x4*>(a.zero + 4 * (tid & 63));
  const int ci = a.cls[ig];
  RowStat st{kNegInf, 0.0f, 0.0f};

  const int t_end = (chunk + 1) * a.per < a.rt ? (chunk + 1) * a.per : a.rt;
  for (int t = chunk * a.per; t < t_end; ++t) {
    const int j0 = kTile * t;
    __syncthreads();      // the previous tile's operand reads are done
    dad_gram_stage(bt, a.z, mu4, j0, a.npad, tid);
    if (tid < kTile) cls_s[tid] = a.cls[j0 + tid];
    __syncthreads();
    const f32x16 acc = scl_gram_block(av, bt, 32 * g.ch, g.l32, g.kh);
    float u[16], tm = kNegInf;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ac = 32 * g.ch + dad_acc_row(r, g.kh), ca = cls_s[ac];
      const bool valid = ca >= 0 && j0 + ac != ig;
      u[r] = valid ? acc[r] * a.inv_tau : kNegInf;
      tm = fmaxf(tm, u[r]);
      // (the very s / tau the log-sum-exp takes: a row whose only other member is its positive has loss exactly 0)
      st.ps += valid && ca == ci ? u[r] : 0.0f;
    }
    const float mn = fmaxf(st.m, tm);
    if (mn > kNegInf) {
      float l = st.l * scl_exp(st.m - mn);
#pragma unroll
      for (int r = 0; r < 16; ++r) l += scl_exp(u[r] - mn);     // (exp(-inf) = 0 for the entries left out)
      st.l = l;
      st.m = mn;
    }
  }
  // the other lane half's 16 columns of every tile, then the other column half's
  st = scl_join(st, RowStat{__shfl_xor(st.m, 32, 64), __shfl_xor(st.l, 32, 64), __shfl_xor(st.ps, 32, 64)});
  if (g.kh == 0) *reinterpret_cast<f32x4*>(&red[g.ch][il][0]) = f32x4{st.m, st.l, st.ps, 0.0f};
  __syncthreads();
  if (tid < kTile) {
    const RowStat r = scl_join(RowStat{red[0][tid][0], red[0][tid][1], red[0][tid][2]},
                               RowStat{red[1][tid][0], red[1][tid][1], red[1][tid][2]});
    *reinterpret_cast<f32x4*>(a.part1 + ((size_t)chunk * a.npad + i0 + tid) * 4) = f32x4{r.m, r.l, r.ps, 0.0f};
  }
}

__global__ __launch_bounds__(kThreads) void dad_scl_pass2(SclArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ float gs[kTile * kGsLd];        // the G tile, [column a][row i]
  __shared__ int cls_s[kTile];
  __shared__ float lse_s[kTile];
  __shared__ float vv_s[DAD_C], cc_s[DAD_C];
  const int tid = threadIdx.x;
  const GramLane g = dad_gram_lane(tid);
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y;
  const int il = 32 * g.rh + g.l32, ig = i0 + il;
  if (tid < DAD_C) {
    const int nc = scl_count(a.cnt, a.rt, tid);
    vv_s[tid] = nc >= 2 ? 1.0f : 0.0f;
    cc_s[tid] = nc >= 2 ? 1.0f / (float)(nc - 1) : 0.0f;
  }
  f32x4 av[DAD_H / 8];
  dad_gram_load_a(av, a.z, a.zero, ig, a.npad, g.kh);
  const f32x4 mu4 = *reinterpret_cast<const f32x4*>(a.zero + 4 * (tid & 63));
  const int ci = a.cls[ig];
  const float lse_i = scl_lse(scl_row_stat(a.part1, a.chunks, a.npad, ig));
  __syncthreads();
  const float vi = ci >= 0 ? vv_s[ci] : 0.0f, cci = ci >= 0 ? cc_s[ci] : 0.0f;
  f32x16 gz[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) gz[cb] = f32x16{};

  const int t_end = (chunk + 1) * a.per < a.rt ? (chunk + 1) * a.per : a.rt;
  for (int t = chunk * a.per; t < t_end; ++t) {
    const int j0 = kTile * t;
    __syncthreads();      // the previous tile's reads of bt, gs and the column tables are done
    dad_gram_stage(bt, a.z, mu4, j0, a.npad, tid);
    if (tid < kTile) {
      cls_s[tid] = a.cls[j0 + tid];
      lse_s[tid] = scl_lse(scl_row_stat(a.part1, a.chunks, a.npad, j0 + tid));
    }
    __syncthreads();
    const f32x16 acc = scl_gram_block(av, bt, 32 * g.ch, g.l32, g.kh);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ac = 32 * g.ch + dad_acc_row(r, g.kh), ca = cls_s[ac];
      const bool valid = ci >= 0 && ca >= 0 && j0 + ac != ig;
      const int ck = ca >= 0 ? ca : 0;
      const float u = acc[r] * a.inv_tau;
      const bool same = ca == ci;
      const float hia = vi * scl_exp(u - lse_i) - (same ? cci : 0.0f);
      const float hai = vv_s[ck] * scl_exp(u - lse_s[ac]) - (same ? cc_s[ck] : 0.0f);
      gs[ac * kGsLd + il] = valid ? hia + hai : 0.0f;
    }
    __syncthreads();
    // rows 32 rh .. of G against the staged rows' columns 128 ch ..: MFMA step s contracts columns a = 2 s, 2 s + 1
#pragma unroll 4
    for (int s = 0; s < kTile / 2; ++s) {
      const int ak = 2 * s + g.kh;
      const float ga = gs[ak * kGsLd + il];
      const float* zb = &bt[ak * kGramLd + 128 * g.ch + g.l32];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) gz[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, zb[32 * cb], gz[cb], 0, 0, 0);
    }
  }
  float* out = a.part2 + ((size_t)chunk * a.npad + i0 + 32 * g.rh) * DAD_H + 128 * g.ch + g.l32;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)dad_acc_row(r, g.kh) * DAD_H + 32 * cb] = gz[cb][r];
}

__global__ __launch_bounds__(kThreads) void dad_scl_final(SclArgs a, SclDst d) {
  __shared__ double red[kThreads];
  __shared__ int nc_s[8];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, i0 = kTile * tile;
  if (tid < 5) nc_s[tid] = scl_count(a.cnt, a.rt, tid);
  __syncthreads();
  int V = 0;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) V += nc_s[c] >= 2 ? nc_s[c] : 0;
  const float scale = V > 0 ? a.inv_tau / (float)V : 0.0f;

  for (int rr = w; rr < kTile; rr += kThreads / 64) {
    const int i = i0 + rr;             // (uniform in the wave)
    if (i >= a.n) break;
    const bool member = a.cls[i] >= 0;
    f32x4 gr = f32x4{};
    if (member) {
      f32x4 gzv = f32x4{};
      for (int q = 0; q < a.chunks; ++q)
        gzv += *reinterpret_cast<const f32x4*>(a.part2 + ((size_t)q * a.npad + i) * DAD_H + 4 * lane);
      gzv *= scale;
      const f32x4 zv = *reinterpret_cast<const f32x4*>(a.z + (size_t)i * DAD_H + 4 * lane);
      double p = 0.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) p += (double)zv[e] * (double)gzv[e];
      const float dot = (float)dad_wave_sum_d(p);
      gr = (gzv - zv * dot) * a.invn[i];
    }
    if (d.grad) *reinterpret_cast<f32x4*>(d.grad + (size_t)i * DAD_H + 4 * lane) = gr;
    if (d.acc && member) {
      const uint32_t ef = d.eflag[i];  // (every lane reads the flag before lane 0 sets it)
      float* dst = d.acc + (size_t)i * DAD_H + 4 * lane;
      const f32x4 old = ef ? *reinterpret_cast<const f32x4*>(dst) : f32x4{};
      *reinterpret_cast<f32x4*>(dst) = old + gr * d.w;
      if (lane == 0) d.eflag[i] = 1u;
    }
  }
  if (tile != 0) return;
  // the anchors' losses: thread tid takes rows tid, tid + 256, ..., thread 0 adds the 256 sums in order
  double s = 0.0;
  for (int i = tid; i < a.n; i += kThreads) {
    const int c = a.cls[i];
    if (c < 0 || nc_s[c] < 2) continue;
    const RowStat st = scl_row_stat(a.part1, a.chunks, a.npad, i);
    const double lse = (double)st.m + log((double)st.l);
    s += lse - (double)st.ps / (double)(nc_s[c] - 1);
  }
  red[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int k = 0; k < kThreads; ++k) tot += red[k];
    const float loss = V > 0 ? (float)(tot / (double)V) : 0.0f;
    if (d.loss) *d.loss = loss;
    if (d.out) {
      d.out[DAD_SCL_LOSS] = loss;
      d.out[DAD_SCL_V] = (float)V;
      d.out[DAD_SCL_MEMBERS] = (float)(((nc_s[0] + nc_s[1]) + nc_s[2]) + nc_s[3]);
      for (int c = 0; c < DAD_C; ++c) d.out[DAD_SCL_ANCHORS + c] = nc_s[c] >= 2 ? (float)nc_s[c] : 0.0f;
      d.out[DAD_SCL_NONFINITE] = (float)nc_s[4];
    }
  }
}

size_t scl_ws_bytes(int64_t n) { return scl_ws_layout(n).bytes; }

SclPlan scl_plan_chunks(int64_t n, int chunks) {
  const PairPlan p = pair_plan(n, chunks, DAD_SCL_MAX_CHUNKS);
  return SclPlan{p.rt, p.chunks, p.per};
}
SclPlan scl_plan_of(int64_t n, int cus) { return scl_plan_chunks(n, cus / (int)((n + kTile - 1) / kTile)); }

int scl_enqueue(const SclSrc& src, const SclDst& dst, float tau, const SclPlan& pl, void* ws, hipStream_t stream) {
  const int n = src.na + src.nb;
  const SclWs L = scl_ws_layout(n);
  SclArgs a;
  float* z = ws_ptr<float>(ws, L.z);
  int32_t* cls = ws_ptr<int32_t>(ws, L.cls);
  float *invn = ws_ptr<float>(ws, L.invn), *zero = ws_ptr<float>(ws, L.zero);
  int32_t* cnt = ws_ptr<int32_t>(ws, L.cnt);
  a.z = z; a.cls = cls; a.invn = invn; a.zero = zero; a.cnt = cnt;
  a.part1 = ws_ptr<float>(ws, L.part1); a.part2 = ws_ptr<float>(ws, L.part2);
  a.n = n; a.npad = pl.rt * kTile; a.rt = pl.rt; a.per = pl.per; a.chunks = pl.chunks;
  a.inv_tau = 1.0f / tau;
  hipLaunchKernelGGL(dad_scl_prep, dim3(pl.rt), dim3(kThreads), 0, stream, src, z, cls, invn, zero, cnt);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_scl_pass1, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, a);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_scl_pass2, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, a);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_scl_final, dim3(pl.rt), dim3(kThreads), 0, stream, a, dst);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_scl_plan(int64_t n, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  if (!row_tiles || !chunks || !tiles_per_chunk) return DAD_E_ARG;
  if (n < 1 || n > DAD_SCL_MAX_N || cus < 1) return DAD_E_SHAPE;
  const SclPlan p = scl_plan_of(n, cus);
  return pair_plan_out(PairPlan{p.rt, p.chunks, p.per}, row_tiles, chunks, tiles_per_chunk);
}

extern "C" size_t dad_scl_workspace_bytes(int64_t n) {
  if (n < 1 || n > DAD_SCL_MAX_N) return 0;
  return scl_ws_bytes(n);
}

extern "C" int dad_scl_chunked(const float* emb, const int64_t* labels, const uint8_t* member, int64_t n, float tau,
                               float* out, float* grad, int chunks, void* ws, void* stream) {
  if (!emb || !labels || !member || !out || !ws || !scl_tau_ok(tau)) return DAD_E_ARG;
  if (n < 1 || n > DAD_SCL_MAX_N) return DAD_E_SHAPE;
  SclPlan pl = scl_plan_chunks(n, chunks);
  if (chunks <= 0) {
    int cus = 0;
    DAD_RET(device_cus(&cus));
    pl = scl_plan_of(n, cus);
  }
  const SclSrc src{emb, labels, member, (int)n, nullptr, nullptr, nullptr, 0};
  const SclDst dst{out, nullptr, grad, nullptr, nullptr, 0.0f};
  return scl_enqueue(src, dst, tau, pl, ws, (hipStream_t)stream);
}

extern "C" int dad_scl(const float* emb, const int64_t* labels, const uint8_t* member, int64_t n, float tau, float* out,
                       float* grad, void* workspace, void* stream) {
  return dad_scl_chunked(emb, labels, member, n, tau, out, grad, 0, workspace, stream);
}
