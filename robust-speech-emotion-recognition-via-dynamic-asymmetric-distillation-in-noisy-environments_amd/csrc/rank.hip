// Rank a split by a key and count positives along the order: risk-coverage, ROC, average precision, the acceptance
// counts of a threshold, torch.quantile and reliability bins, for up to 16 columns of up to 65,536 rows.
//
// The split-wide, multi-column form of the rank-by-counting that dacp_thresholds (tail_common.h) does for one batch:
// DACP keeps a pseudo-label when the teacher's certainty score clears a per-class quantile (I/utils.py:449-507), and
// every question about that gate is "order the rows by the score and count along the order".  include/dad.h has the
// meaning of every output.  Row i takes part in column j when its member bit is set and key[j][i] is finite; the
// order is (key descending, row index ascending) with keys compared as values (-0.0 == +0.0).
//
// Three launches behind each other on the stream, no floating-point atomics, no counter between workgroups:
//
//   dad_rank_count    workgroup (row tile, chunk, column): 256 rows, one per thread, against a contiguous run of
//                     256-key tiles of the same column.  A tile's keys are staged in LDS, NaN in place of a row that
//                     does not take part (no comparison with NaN holds, so such a row is counted by nobody); every
//                     thread reads them by broadcast, four per 16-byte read, and counts the rows that precede its
//                     own.  The count of chunk c goes to part[c][j][i]: an integer, exact.
//   dad_rank_scatter  one thread per (row, column): the rank is the sum of the chunks' counts.  Ranks of a column are a
//                     permutation of 0 .. M-1, so the writes of key, positive flag and row index to position `rank`
//                     never collide.  Zeros are stored as +0.0, so nothing downstream sees which zero a row held.
//   dad_rank_finish   one workgroup of 256 threads per column, whatever n and the chunk count are.  Thread t owns
//                     the positions [t E, (t+1) E), E = ceil(n / 256): it counts its positives and finds its last
//                     tie end, the threads' counts are prefixed in thread order, and a second walk writes cum_pos,
//                     tie_end and, per tie end, the tie end before it.  All integers.  Every double is then
//                     block_sum over the positions: thread t adds positions lo + t, lo + t + 256, ... in that
//                     order, and the 256 partial sums meet in a fixed binary tree.  That order is a function of the
//                     sorted sequence alone: not of the grid, the chunk count or the order of the rows.
//
// Work per call: m n^2 compares in dad_rank_count (four VALU operations each), 4 m n bytes of counts per chunk.
#include <cmath>
#include <cstdint>

#include "dad_common.h"

namespace {

constexpr int kThreads = DAD_RK_TILE;          // rows of a row tile = keys of a key tile = threads of every kernel
constexpr int kMaxChunks = DAD_RK_MAX_CHUNKS;

static_assert(kThreads == 256 && DAD_RK_MAX_BINS <= kThreads && DAD_RK_MAX_Q <= kThreads, "the finishing workgroup");

struct RankWs {
  size_t part, skey, sflag, cum, tie, prev, bytes;
};

// (a function of n and m alone: a call runs with at most min(key tiles, kMaxChunks) chunks)
RankWs rank_ws_layout(int64_t n, int m) {
  RankWs w;
  const size_t ct = (size_t)((n + kThreads - 1) / kThreads), cells = (size_t)m * (size_t)n;
  const size_t maxc = ct < (size_t)kMaxChunks ? ct : (size_t)kMaxChunks;
  size_t off = 0;
  w.part = off;  off = dad_align(off + sizeof(int32_t) * maxc * cells);
  w.skey = off;  off = dad_align(off + sizeof(float) * cells);
  w.sflag = off; off = dad_align(off + sizeof(uint8_t) * cells);
  w.cum = off;   off = dad_align(off + sizeof(int32_t) * cells);
  w.tie = off;   off = dad_align(off + sizeof(uint8_t) * cells);
  w.prev = off;  off = dad_align(off + sizeof(int32_t) * cells);
  w.bytes = off;
  return w;
}

struct RankPlan {
  int rt, chunks, per;
};

RankPlan rank_plan(int64_t n, int want) {
  RankPlan p;
  p.rt = (int)((n + kThreads - 1) / kThreads);
  const int cap = p.rt < kMaxChunks ? p.rt : kMaxChunks;
  want = want < 1 ? 1 : (want > cap ? cap : want);
  p.per = (p.rt + want - 1) / want;
  p.chunks = (p.rt + p.per - 1) / p.per;
  return p;
}

bool rank_shape_ok(int64_t n, int m) { return n >= 1 && n <= DAD_RK_MAX_N && m >= 1 && m <= DAD_RK_MAX_M; }

// the key a row is ranked by: NaN when it does not take part
__device__ __forceinline__ float rank_key(float k, uint8_t f) {
  return (f & DAD_RK_MEMBER) && fabsf(k) < INFINITY ? k : NAN;
}

// The sum of f(k) over k in [lo, hi) by the whole workgroup, in an order that depends on lo and hi alone: thread t
// adds k = lo + t, lo + t + 256, ..., then the partial sums meet in a binary tree.  Every thread returns the sum.
template <typename F>
__device__ __forceinline__ double block_sum(int lo, int hi, double* red, F f) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = lo + tid; k < hi; k += kThreads) s += f(k);
  __syncthreads();          // (red may still be read from the sum before)
  red[tid] = s;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  return red[0];
}

}  // namespace

__global__ __launch_bounds__(kThreads) void dad_rank_count(const float* __restrict__ key,
                                                           const uint8_t* __restrict__ flags,
                                                           int32_t* __restrict__ part, int n, int m, int ct, int per) {
  __shared__ __attribute__((aligned(16))) float ks[kThreads];
  const int tid = threadIdx.x, chunk = blockIdx.y, j = blockIdx.z;
  const int i = kThreads * (int)blockIdx.x + tid;
  const float* kj = key + (size_t)j * n;
  const uint8_t* fj = flags + (size_t)j * n;
  const float kv = i < n ? rank_key(kj[i], fj[i]) : NAN;
  const int t1 = (chunk + 1) * per < ct ? (chunk + 1) * per : ct;
  int cnt = 0;
  for (int t = chunk * per; t < t1; ++t) {
    const int k0 = kThreads * t, kk = k0 + tid;
    __syncthreads();
    ks[tid] = kk < n ? rank_key(kj[kk], fj[kk]) : NAN;
    __syncthreads();
#pragma unroll 4
    for (int u = 0; u < kThreads; u += 4) {
      const float4 o = *reinterpret_cast<const float4*>(&ks[u]);
      const int k = k0 + u;
      cnt += (o.x > kv || (o.x == kv && k < i)) ? 1 : 0;
      cnt += (o.y > kv || (o.y == kv && k + 1 < i)) ? 1 : 0;
      cnt += (o.z > kv || (o.z == kv && k + 2 < i)) ? 1 : 0;
      cnt += (o.w > kv || (o.w == kv && k + 3 < i)) ? 1 : 0;
    }
  }
  if (i < n) part[((size_t)chunk * m + j) * n + i] = cnt;
}

__global__ __launch_bounds__(kThreads) void dad_rank_scatter(const float* __restrict__ key,
                                                             const uint8_t* __restrict__ flags,
                                                             const int32_t* __restrict__ part, int n, int m, int chunks,
                                                             float* __restrict__ skey, uint8_t* __restrict__ sflag,
                                                             int32_t* __restrict__ order) {
  const int i = kThreads * (int)blockIdx.x + (int)threadIdx.x, j = blockIdx.y;
  if (i >= n) return;
  const size_t cj = (size_t)j * n;
  const uint8_t f = flags[cj + i];
  const float kv = rank_key(key[cj + i], f);
  if (!(kv == kv)) return;
  int r = 0;
  for (int c = 0; c < chunks; ++c) r += part[((size_t)c * m + j) * n + i];
  skey[cj + r] = kv + 0.0f;         // (-0.0 + 0.0 = +0.0: one zero)
  sflag[cj + r] = (f & DAD_RK_POSITIVE) ? 1 : 0;
  if (order) order[cj + r] = i;
}

struct RankFinishArgs {
  const float* key;
  const uint8_t* flags;
  const float* thr;
  const float* gammas;
  const float* skey;
  const uint8_t* sflag;
  int32_t* cum;        // cum_pos or the workspace's
  uint8_t* tie;        // tie_end or the workspace's
  int32_t* prev;       // workspace: at a tie end, the tie end before it (-1: none)
  int32_t* order;      // or NULL
  int64_t* counts;
  double* values;
  float* quant;
  int64_t* bin_counts;
  double* bin_sum;
  int n, Q, B;
  float bin_lo, bin_hi;
};

__global__ __launch_bounds__(kThreads) void dad_rank_finish(RankFinishArgs a) {
  __shared__ double red[kThreads];
  __shared__ int seg_pos[kThreads], seg_te[kThreads], seg_cte[kThreads];
  __shared__ int tot[4];                       // members, positives, non-finite, M
  __shared__ int acc[3];                       // runs, accepted, accepted positives
  __shared__ unsigned long long u2_s;
  __shared__ int bc[DAD_RK_MAX_BINS], bp[DAD_RK_MAX_BINS];
  const int tid = threadIdx.x, j = blockIdx.x, n = a.n;
  const size_t cj = (size_t)j * n;
  const float* skey = a.skey + cj;
  const uint8_t* sflag = a.sflag + cj;
  int32_t* cum = a.cum + cj;
  uint8_t* tie = a.tie + cj;
  int32_t* prev = a.prev + cj;

  if (tid < 4) tot[tid] = 0;
  if (tid < 3) acc[tid] = 0;
  if (tid == 0) u2_s = 0ull;
  if (tid < DAD_RK_MAX_BINS) bc[tid] = bp[tid] = 0;
  __syncthreads();
  {
    int mem = 0, pos = 0, bad = 0, part = 0;
    for (int i = tid; i < n; i += kThreads) {
      const uint8_t f = a.flags[cj + i];
      if (!(f & DAD_RK_MEMBER)) continue;
      ++mem;
      if (fabsf(a.key[cj + i]) < INFINITY) {
        ++part;
        pos += (f & DAD_RK_POSITIVE) ? 1 : 0;
      } else {
        ++bad;
      }
    }
    atomicAdd(&tot[0], mem);
    atomicAdd(&tot[1], pos);
    atomicAdd(&tot[2], bad);
    atomicAdd(&tot[3], part);
  }
  __syncthreads();
  const int M = tot[3], P = tot[1], N = M - P;
  const float thr = a.thr[j];

  // the thread's positions, first walk: positives, the last tie end and the positives up to it, runs, acceptance
  const int E = (n + kThreads - 1) / kThreads;
  const int s0 = tid * E < n ? tid * E : n, s1 = s0 + E < n ? s0 + E : n;
  const int m1 = s1 < M ? s1 : M;              // positions [s0, m1) hold rows, [max(s0, M), s1) are behind them
  {
    int lp = 0, lte = -1, lcte = 0, runs = 0, ac = 0, acp = 0;
    for (int k = s0; k < m1; ++k) {
      const float v = skey[k];
      const int p = sflag[k];
      lp += p;
      const bool te = k == M - 1 || skey[k + 1] != v;
      tie[k] = te ? 1 : 0;
      if (te) { lte = k; lcte = lp; ++runs; }
      if (v >= thr) { ++ac; acp += p; }
    }
    for (int k = s0 > M ? s0 : M; k < s1; ++k) {
      tie[k] = 0;
      cum[k] = 0;
      if (a.order) a.order[cj + k] = -1;
    }
    seg_pos[tid] = lp;
    seg_te[tid] = lte;
    seg_cte[tid] = lcte;
    atomicAdd(&acc[0], runs);
    atomicAdd(&acc[1], ac);
    atomicAdd(&acc[2], acp);
  }
  __syncthreads();
  {
    // the threads before this one, in thread order: positives so far, the last tie end and cum_pos there
    int c = 0, pte = -1, cpte = 0;
    for (int t = 0; t < tid; ++t) {
      if (seg_te[t] >= 0) { pte = seg_te[t]; cpte = c + seg_cte[t]; }
      c += seg_pos[t];
    }
    unsigned long long u2 = 0ull;
    for (int k = s0; k < m1; ++k) {
      c += sflag[k];
      cum[k] = c;
      if (tie[k]) {
        prev[k] = pte;
        const long long pos_r = c - cpte, size_r = k - pte, neg_r = size_r - pos_r;
        const long long below = (long long)N - ((long long)(k + 1) - c);     // negatives with a smaller key
        u2 += (unsigned long long)(pos_r * (2 * below + neg_r));
        pte = k;
        cpte = c;
      }
    }
    atomicAdd(&u2_s, u2);
  }
  __threadfence_block();
  __syncthreads();

  // the doubles: each a block_sum over positions
  const double dM = (double)M, dP = (double)P;
  const double ksum = block_sum(0, M, red, [&](int k) { return (double)skey[k]; });
  const double mean = M > 0 ? ksum / dM : 0.0;
  const double kvar = block_sum(0, M, red, [&](int k) {
    const double d = (double)skey[k] - mean;
    return d * d;
  });
  const double ap = block_sum(0, M, red, [&](int k) {
    if (!tie[k] || P == 0) return 0.0;
    const int pk = prev[k];
    const double c = (double)cum[k], cp = pk >= 0 ? (double)cum[pk] : 0.0;
    return (c / dP - cp / dP) * (c / (double)(k + 1));
  });
  const double rc = block_sum(0, M, red, [&](int k) {
    if (!tie[k]) return 0.0;
    const double taken = (double)(k + 1);
    return (double)(k - prev[k]) * ((taken - (double)cum[k]) / taken);
  });

  // reliability bins: a bin's rows are contiguous in the order (the bin index does not decrease with the key)
  const int B = a.B;
  if (B > 0) {
    const double lo = (double)a.bin_lo, width = (double)a.bin_hi - (double)a.bin_lo;
    for (int k = tid; k < M; k += kThreads) {
      const double v = floor(((double)skey[k] - lo) / width * (double)B);
      const int b = v < 0.0 ? 0 : (v > (double)(B - 1) ? B - 1 : (int)v);
      atomicAdd(&bc[b], 1);
      atomicAdd(&bp[b], (int)sflag[k]);
    }
    __syncthreads();
    int start = 0;
    for (int b = B - 1; b >= 0; --b) {        // (descending keys: the last bin comes first)
      const int cb = bc[b];
      const double s = block_sum(start, start + cb, red, [&](int k) { return (double)skey[k]; });
      if (tid == 0) {
        a.bin_counts[((size_t)j * B + b) * 2 + 0] = cb;
        a.bin_counts[((size_t)j * B + b) * 2 + 1] = bp[b];
        a.bin_sum[(size_t)j * B + b] = s;
      }
      start += cb;
    }
  }

  if (tid < a.Q) {
    // torch.quantile(linear) in float32, the arithmetic of dacp_class_threshold (tail_common.h)
    float q = NAN;
    if (M > 0) {
      const float rank = a.gammas[tid] * (float)(M - 1);
      int lo = (int)rank, hi = (int)ceilf(rank);
      const float wgt = rank - (float)lo;
      lo = lo < 0 ? 0 : (lo > M - 1 ? M - 1 : lo);
      hi = hi < 0 ? 0 : (hi > M - 1 ? M - 1 : hi);
      const float vlo = skey[M - 1 - lo], vhi = skey[M - 1 - hi];
      q = wgt < 0.5f ? vlo + wgt * (vhi - vlo) : vhi - (vhi - vlo) * (1.0f - wgt);
    }
    a.quant[(size_t)j * a.Q + tid] = q;
  }
  if (tid == 0) {
    const bool has_thr = thr == thr;
    const bool valid = P > 0 && N > 0;
    int64_t* c = a.counts + (size_t)j * DAD_RK_COUNTS;
    c[DAD_RK_MEMBERS] = M;
    c[DAD_RK_POSITIVES] = P;
    c[DAD_RK_NONFINITE] = tot[2];
    c[DAD_RK_RUNS] = acc[0];
    c[DAD_RK_U2] = (int64_t)u2_s;
    c[DAD_RK_ACCEPTED] = has_thr ? acc[1] : 0;
    c[DAD_RK_ACCEPTED_POS] = has_thr ? acc[2] : 0;
    c[DAD_RK_VALID_AUROC] = valid ? 1 : 0;
    double* v = a.values + (size_t)j * DAD_RK_VALUES;
    v[DAD_RK_AUROC] = valid ? (double)(int64_t)u2_s / (2.0 * dP * (double)N) : 0.0;
    v[DAD_RK_AP] = ap;
    v[DAD_RK_AURC] = M > 0 ? rc / dM : 0.0;
    v[DAD_RK_KEY_MEAN] = mean;
    v[DAD_RK_KEY_STD] = M > 0 ? sqrt(kvar / dM) : 0.0;
    v[DAD_RK_KEY_MIN] = M > 0 ? (double)skey[M - 1] : 0.0;
    v[DAD_RK_KEY_MAX] = M > 0 ? (double)skey[0] : 0.0;
    v[DAD_RK_VALUES - 1] = 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void dad_rank_columns(const float* __restrict__ score,
                                                             const float* __restrict__ probs,
                                                             const int64_t* __restrict__ pred,
                                                             const int64_t* __restrict__ labels, int n,
                                                             float* __restrict__ key, uint8_t* __restrict__ flags) {
  const int i = kThreads * (int)blockIdx.x + (int)threadIdx.x;
  if (i >= n) return;
  const int64_t p = pred[i], y = labels ? labels[i] : 0;
  const bool in = p >= 0 && p < DAD_C && y >= 0 && y < DAD_C;
  const bool right = labels && p == y;
  const float s = score[i];
  float pc[DAD_C], pmax = probs[(size_t)i * DAD_C];
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    pc[c] = probs[(size_t)i * DAD_C + c];
    pmax = pc[c] > pmax ? pc[c] : pmax;
  }
  const uint8_t member = in ? DAD_RK_MEMBER : 0, hit = in && right ? DAD_RK_POSITIVE : 0;
  key[i] = s;
  flags[i] = member | hit;
  key[(size_t)5 * n + i] = pmax;
  flags[(size_t)5 * n + i] = member | hit;
#pragma unroll
  for (int c = 0; c < DAD_C; ++c) {
    const uint8_t is_c = in && labels && y == c ? DAD_RK_POSITIVE : 0;
    key[(size_t)(1 + c) * n + i] = s;
    flags[(size_t)(1 + c) * n + i] = (in && p == c ? DAD_RK_MEMBER : 0) | is_c;
    key[(size_t)(6 + c) * n + i] = pc[c];
    flags[(size_t)(6 + c) * n + i] = member | is_c;
  }
}

extern "C" int dad_rank_plan(int64_t n, int m, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  if (!row_tiles || !chunks || !tiles_per_chunk) return DAD_E_ARG;
  if (!rank_shape_ok(n, m) || cus < 1) return DAD_E_SHAPE;
  // four workgroups of the counting pass a compute unit (256 threads and 1 KB of LDS each), if the key tiles allow
  const int64_t wgs = (int64_t)((n + kThreads - 1) / kThreads) * m;
  const RankPlan p = rank_plan(n, (int)((4 * (int64_t)cus + wgs - 1) / wgs));
  *row_tiles = p.rt;
  *chunks = p.chunks;
  *tiles_per_chunk = p.per;
  return DAD_OK;
}

extern "C" size_t dad_rank_workspace_bytes(int64_t n, int m) {
  if (!rank_shape_ok(n, m)) return 0;
  return rank_ws_layout(n, m).bytes;
}

extern "C" int dad_rank_metrics_chunked(const dad_rank_args* a, int chunks, void* ws, void* stream_) {
  if (!a || !ws || !a->key || !a->flags || !a->thr || !a->counts || !a->values) return DAD_E_ARG;
  if (!rank_shape_ok(a->n, a->m) || a->Q < 0 || a->Q > DAD_RK_MAX_Q || a->B < 0 || a->B > DAD_RK_MAX_BINS)
    return DAD_E_SHAPE;
  if (a->Q > 0 && (!a->gammas || !a->quant)) return DAD_E_ARG;
  if (a->B > 0 && (!a->bin_counts || !a->bin_sum || !(a->bin_lo < a->bin_hi) || !std::isfinite(a->bin_lo) ||
                   !std::isfinite(a->bin_hi)))
    return DAD_E_ARG;
  const int n = (int)a->n, m = a->m;
  RankPlan pl;
  if (chunks > 0) {
    pl = rank_plan(n, chunks);
  } else {
    int cus = 0;
    DAD_RET(device_cus(&cus));
    DAD_RET(dad_rank_plan(n, m, cus, &pl.rt, &pl.chunks, &pl.per));
  }
  hipStream_t stream = (hipStream_t)stream_;
  const RankWs L = rank_ws_layout(n, m);
  int32_t* part = ws_ptr<int32_t>(ws, L.part);
  float* skey = ws_ptr<float>(ws, L.skey);
  uint8_t* sflag = ws_ptr<uint8_t>(ws, L.sflag);

  hipLaunchKernelGGL(dad_rank_count, dim3(pl.rt, pl.chunks, m), dim3(kThreads), 0, stream, a->key, a->flags, part, n, m,
                     pl.rt, pl.per);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_rank_scatter, dim3(pl.rt, m), dim3(kThreads), 0, stream, a->key, a->flags, part, n, m,
                     pl.chunks, skey, sflag, a->order);
  DAD_TRY(hipGetLastError());
  RankFinishArgs f;
  f.key = a->key; f.flags = a->flags; f.thr = a->thr; f.gammas = a->gammas; f.skey = skey; f.sflag = sflag;
  f.cum = a->cum_pos ? a->cum_pos : ws_ptr<int32_t>(ws, L.cum);
  f.tie = a->tie_end ? a->tie_end : ws_ptr<uint8_t>(ws, L.tie);
  f.prev = ws_ptr<int32_t>(ws, L.prev);
  f.order = a->order; f.counts = a->counts; f.values = a->values; f.quant = a->quant;
  f.bin_counts = a->bin_counts; f.bin_sum = a->bin_sum;
  f.n = n; f.Q = a->Q; f.B = a->B; f.bin_lo = a->bin_lo; f.bin_hi = a->bin_hi;
  hipLaunchKernelGGL(dad_rank_finish, dim3(m), dim3(kThreads), 0, stream, f);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_rank_metrics(const dad_rank_args* a, void* workspace, void* stream) {
  return dad_rank_metrics_chunked(a, 0, workspace, stream);
}

extern "C" int dad_rank_eval_columns(const float* score, const float* probs, const int64_t* pred, const int64_t* labels,
                                     int64_t n, float* key, uint8_t* flags, void* stream) {
  if (!score || !probs || !pred || !key || !flags) return DAD_E_ARG;
  if (n < 1 || n > DAD_RK_MAX_N) return DAD_E_SHAPE;
  hipLaunchKernelGGL(dad_rank_columns, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, score, probs, pred, labels, (int)n, key, flags);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}
