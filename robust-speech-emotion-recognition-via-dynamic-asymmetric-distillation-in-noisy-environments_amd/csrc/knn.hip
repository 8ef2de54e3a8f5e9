// Exact k nearest neighbours of a split's embeddings on the device, and the three scores built on them: the uniform
// k-NN vote, cross-group retrieval (one call with the domain as the group) and scikit-learn's trustworthiness of a
// 2-D map (include/dad.h restates the semantics).  No floating-point atomics anywhere; selection is by a total order
// on bits that do not depend on the chunking, so every chunk count gives the same output bits.
//
//   dad_knn
//     dad_pair_prep      (pairwise.hip, one group: the rows with group >= 0) one workgroup per 64-row tile: the
//                        participating rows' column sums in double, their count and the count of those with a
//                        non-finite component
//     dad_pair_mean      (pairwise.hip) one workgroup: the tiles in tile order -> the participating rows' mean
//                        rounded to fp32, the counts into the workspace's first words
//     dad_pair_norms     (pairwise.hip) |x_i - mu|^2 as the diagonal of the Gram block
//     dad_knn_pair       pairwise.h's walk.  Workgroup (row tile, chunk).  The walk's epilogue puts the tile's
//                        dad_pair_d2 into LDS -- into bt itself, behind a barrier that ends every wave's operand reads
//                        -- and behind a second barrier four lanes per row mark the columns that are candidates below
//                        the row's last key.  A candidate is the key (d2 bits << 32 | j), which orders as the pair
//                        (d2, j) because d2 >= 0.  Behind a third barrier lane = row of the first wave puts its marked
//                        columns into the row's ascending k-list in LDS.  The chunk's lists go to the workspace.
//     dad_knn_merge      lane = row: the chunks' lists through the same insertion -> idx, d2
//   dad_knn_vote         a launch that clears the block, then lane = row: the labels of the row's neighbours, the first
//                        maximum; the confusion block by integer atomics (LDS, then one global add per slot and
//                        workgroup)
//   dad_trustworthiness
//     prep, mean, norms as above over all rows
//     dad_knn_y          lane = row: the k nearest rows of Y by the same key, from the fp32 differences
//     dad_knn_gather     one wave per 32 rows: D_ij of the row's k map neighbours as the diagonal of a Gram block
//                        whose B operand is the neighbours' rows (the same operand values through the same chain of
//                        128 MFMAs as the walk's entry (i, j): the same bits) -> the keys (D_ij, j)
//     dad_knn_count      the walk again, chunked: per row and map neighbour, the columns l not in {i, j} whose key
//                        (D_il, l) is below (D_ij, j); four lanes per row, 16 columns each, int32 counts
//     dad_knn_penalty    lane = row: the chunks' counts -> rank, penalty
//     dad_knn_trust      one workgroup: the penalties in int64 -> T in double
//
// LDS: the staged column tile is 66,560 B and two workgroups of a walk share a CU's 160 KiB only below 81,920 B each.
// The d2 tile therefore reuses bt (three extra barriers per column tile in dad_knn_pair, two in dad_knn_count) and
// the lists are sized by a template parameter: up to k = 16 they take 8 KB (12 KB with the counts of dad_knn_count)
// and two workgroups fit; from k = 17 they take 16 KB (24 KB) and one workgroup runs per CU, its staging exposed.
// DESIGN.md 6b has the measured cost.
#include <cmath>
#include <cstdint>

#include "dad_common.h"
#include "pairwise.h"

namespace {

constexpr int kTile = DAD_KNN_TILE;
constexpr int kThreads = kGramThreads;
constexpr int kMaxChunks = DAD_KNN_MAX_CHUNKS;
constexpr int kMaxK = DAD_KNN_MAX_K;
constexpr int kDtLd = kTile + 1;           // row stride of the d2 tile in bt (odd: a column is conflict-free)
constexpr uint64_t kEmpty = ~0ull;         // above every key (a key's high word is at most 0x7fffffff)
constexpr int kHdrBad = DAD_KNN_WS_NONFINITE;

static_assert(kTile == kGramTile && kTile == 64 && DAD_H == 256, "the Gram block's wave / lane mapping");
static_assert(kTile * kDtLd <= kTile * kGramLd, "the d2 tile fits the staged column tile");
static_assert(kHdrBad == kPairHdrBad, "dad_pair_mean writes the non-finite count where include/dad.h promises it");

struct KnnWs {
  size_t hdr, mean, norms, csum, cnt, keys, ynbr, thr, pen, bytes;
};

// (a function of n and k alone; the chunk lists of dad_knn and the chunk counts of dad_trustworthiness share `keys`)
KnnWs knn_ws_layout(int64_t n, int k) {
  KnnWs w;
  const size_t rt = (size_t)((n + kTile - 1) / kTile), npad = rt * kTile;
  const size_t maxc = rt < (size_t)kMaxChunks ? rt : (size_t)kMaxChunks;
  size_t off = 0;
  w.hdr = off;   off = dad_align(off + sizeof(int32_t) * 64);
  w.mean = off;  off = dad_align(off + sizeof(float) * DAD_H);
  w.norms = off; off = dad_align(off + sizeof(float) * npad);
  w.csum = off;  off = dad_align(off + sizeof(double) * rt * DAD_H);
  w.cnt = off;   off = dad_align(off + sizeof(int32_t) * rt * 2);
  w.keys = off;  off = dad_align(off + sizeof(uint64_t) * maxc * npad * (size_t)k);
  w.ynbr = off;  off = dad_align(off + sizeof(int32_t) * npad * (size_t)k);
  w.thr = off;   off = dad_align(off + sizeof(uint64_t) * npad * (size_t)k);
  w.pen = off;   off = dad_align(off + sizeof(int32_t) * npad);
  w.bytes = off;
  return w;
}

// the pair (d2, j) as one integer: d2 >= 0, so its bits order as its value
__device__ __forceinline__ uint64_t knn_key(float d2, int j) {
  return ((uint64_t)(__float_as_uint(d2) & 0x7fffffffu) << 32) | (uint32_t)j;
}

// key into the ascending list list[0], list[stride], ..., k entries, whose last it is below: its place by bisection
// (5 dependent reads at k = 32), then the tail moves up four entries at a time, reads before writes, so that the
// moves do not wait for one another
__device__ __forceinline__ void knn_insert(uint64_t* list, int stride, int k, uint64_t key) {
  int lo = 0, hi = k - 1;            // the first entry above key is in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (list[mid * stride] > key) hi = mid;
    else lo = mid + 1;
  }
  int s = k - 1;
  for (; s - 4 >= lo; s -= 4) {
    const uint64_t a = list[(s - 1) * stride], b = list[(s - 2) * stride], c = list[(s - 3) * stride],
                   d = list[(s - 4) * stride];
    list[s * stride] = a;
    list[(s - 1) * stride] = b;
    list[(s - 2) * stride] = c;
    list[(s - 3) * stride] = d;
  }
  for (; s > lo; --s) list[s * stride] = list[(s - 1) * stride];
  list[lo * stride] = key;
}

// The candidates of one row among 64 columns, bit c of mask = column c, into its list, in column order.  A wave's
// lanes run this side by side, so its time is that of the row with the most candidates, not of every column that is a
// candidate of some row; worst is the list's last key (a candidate that was below it when the mask was made may not
// be any more).
template <typename KeyOf>
__device__ __forceinline__ void knn_take(uint64_t mask, uint64_t* list, int stride, int k, uint64_t& worst,
                                         KeyOf key_of) {
  while (mask) {
    const int c = __builtin_ctzll(mask);
    mask &= mask - 1;
    const uint64_t key = key_of(c);
    if (key < worst) {
      knn_insert(list, stride, k, key);
      worst = list[(k - 1) * stride];
    }
  }
}

__device__ __forceinline__ bool knn_candidate(int mode, int gi, int gj) {
  return gj >= 0 && (mode == DAD_KNN_ALL || (mode == DAD_KNN_SAME ? gj == gi : gj != gi));
}

}  // namespace

struct KnnPairArgs {
  const float* emb;
  const int32_t* group;
  const float* norms;
  const float* mean;
  uint64_t* part;       // [chunks][npad][k]
  int n, npad, ct, per, k, mode;
};

template <int KCAP>
__global__ __launch_bounds__(kThreads, KCAP <= 16 ? 2 : 1) void dad_knn_pair(KnnPairArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ float nj_s[kTile], ni_s[kTile];
  __shared__ int gj_s[kTile], gi_s[kTile];
  __shared__ uint64_t list_s[KCAP * kTile];      // [slot][row]
  __shared__ uint64_t mask_s[kTile];             // per row, 16 bits per quarter of the tile's columns
  const int tid = threadIdx.x;
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y, n = a.n, k = a.k, mode = a.mode;
  if (tid < kTile) gi_s[tid] = i0 + tid < n ? (a.group ? a.group[i0 + tid] : 0) : -1;
  for (int e = tid; e < k * kTile; e += kThreads) list_s[e] = kEmpty;
  uint64_t worst = kEmpty;                       // of lane = row of wave 0
  float* dt = bt;       // the d2 tile [64][kDtLd], between the walk's operand reads and its next staging
  const int row = tid >> 2, q4 = tid & 3;        // the filter: four lanes per row, 16 columns each

  dad_gram_walk_chunk(
      a.emb, a.norms, a.mean, n, i0, chunk, a.per, a.ct, bt, nj_s, ni_s,
      [&](int c, int j) { gj_s[c] = j < n ? (a.group ? a.group[j] : 0) : -1; },
      [&](int r, int ig, int jc, int jg, float d2) {
        if (r == 0) __syncthreads();       // every wave's operand reads of this tile are done
        dt[(ig - i0) * kDtLd + jc] = d2;
        if (r == 15) {
          __syncthreads();
          const int j0 = jg - jc;
          {   // every lane: which of its 16 columns are candidates below the row's last key
            const int gi = gi_s[row], me = i0 + row, c0 = 16 * q4;
            const uint64_t last = list_s[(k - 1) * kTile + row];
            uint32_t m = 0;
#pragma unroll 4
            for (int e = 0; e < 16; ++e) {
              const bool ok = gi >= 0 && knn_candidate(mode, gi, gj_s[c0 + e]) && j0 + c0 + e != me &&
                              knn_key(dt[row * kDtLd + c0 + e], j0 + c0 + e) < last;
              m |= (uint32_t)ok << e;
            }
            reinterpret_cast<uint16_t*>(mask_s)[tid] = (uint16_t)m;      // (little-endian: quarter q4 of row's word)
          }
          __syncthreads();
          if (tid < kTile)
            knn_take(mask_s[tid], list_s + tid, kTile, k, worst,
                     [&](int c) { return knn_key(dt[tid * kDtLd + c], j0 + c); });
        }
      });
  if (tid < kTile)
    for (int s = 0; s < k; ++s) a.part[((size_t)chunk * a.npad + i0 + tid) * k + s] = list_s[s * kTile + tid];
}

__global__ __launch_bounds__(kTile) void dad_knn_merge(const uint64_t* __restrict__ part, int n, int npad, int chunks,
                                                       int k, int32_t* __restrict__ idx, float* __restrict__ d2) {
  __shared__ uint64_t list_s[kMaxK * kTile];
  const int tid = threadIdx.x, row = kTile * (int)blockIdx.x + tid;
  if (row >= n) return;
  uint64_t* list = list_s + tid;
  for (int s = 0; s < k; ++s) list[s * kTile] = kEmpty;
  uint64_t worst = kEmpty;
  for (int q = 0; q < chunks; ++q) {
    const uint64_t* src = part + ((size_t)q * npad + row) * k;
    for (int s = 0; s < k; ++s) {
      const uint64_t key = src[s];
      if (key >= worst) break;       // (ascending: the rest of this chunk's list is no better)
      knn_insert(list, kTile, k, key);
      worst = list[(k - 1) * kTile];
    }
  }
  for (int s = 0; s < k; ++s) {
    const uint64_t key = list[s * kTile];
    idx[(size_t)row * k + s] = key == kEmpty ? -1 : (int32_t)(uint32_t)key;
    d2[(size_t)row * k + s] = key == kEmpty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
  }
}

// ---------------------------------------------------------------------------------- the vote
__global__ __launch_bounds__(64) void dad_knn_vote_clear(unsigned long long* __restrict__ out) {
  if (threadIdx.x < DAD_KV_SLOTS) out[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kThreads) void dad_knn_vote_rows(const int32_t* __restrict__ idx,
                                                              const int64_t* __restrict__ labels,
                                                              const int32_t* __restrict__ group, int n, int k,
                                                              int64_t* __restrict__ pred,
                                                              unsigned long long* __restrict__ out) {
  __shared__ int h_s[DAD_KV_SLOTS];
  const int tid = threadIdx.x, i = kThreads * (int)blockIdx.x + tid;
  if (tid < DAD_KV_SLOTS) h_s[tid] = 0;
  __syncthreads();
  if (i < n) {
    const int g = group ? group[i] : 0;
    int p = -1;
    if (g >= 0) {
      int v[DAD_C] = {0, 0, 0, 0};
      for (int s = 0; s < k; ++s) {
        const int j = idx[(size_t)i * k + s];
        if (j < 0 || j >= n) continue;
        const long lab = labels[j];
#pragma unroll
        for (int c = 0; c < DAD_C; ++c) v[c] += lab == c;
      }
      int best = 0;
#pragma unroll
      for (int c = 0; c < DAD_C; ++c)
        if (v[c] > best) {           // (the first maximum: the smallest class on a tie)
          best = v[c];
          p = c;
        }
    }
    pred[i] = p;
    const long li = labels[i];
    if (g >= 0 && li >= 0 && li < DAD_C) {
      const int gq = g != 0;
      atomicAdd(&h_s[DAD_KV_QUERIES + gq], 1);
      atomicAdd(&h_s[p >= 0 ? DAD_KV_CONFUSION + (gq * DAD_C + (int)li) * DAD_C + p : DAD_KV_NO_VOTE + gq], 1);
    }
  }
  __syncthreads();
  if (tid < DAD_KV_SLOTS && h_s[tid] != 0) atomicAdd(&out[tid], (unsigned long long)h_s[tid]);
}

// ---------------------------------------------------------------------------------- trustworthiness
// the k nearest rows of Y of each row, by (|y_i - y_j|^2, j) from the fp32 differences
__global__ __launch_bounds__(kTile) void dad_knn_y(const float* __restrict__ Y, int n, int k,
                                                   int32_t* __restrict__ ynbr) {
  __shared__ f32x2 ys[kTile];
  __shared__ uint64_t list_s[kMaxK * kTile];
  const int tid = threadIdx.x, row = kTile * (int)blockIdx.x + tid;
  const f32x2* Y2 = reinterpret_cast<const f32x2*>(Y);
  const f32x2 yi = row < n ? Y2[row] : f32x2{0.0f, 0.0f};
  uint64_t* list = list_s + tid;
  for (int s = 0; s < k; ++s) list[s * kTile] = kEmpty;
  uint64_t worst = kEmpty;
  for (int j0 = 0; j0 < n; j0 += kTile) {
    __syncthreads();        // the previous tile's reads are done
    ys[tid] = j0 + tid < n ? Y2[j0 + tid] : f32x2{0.0f, 0.0f};
    __syncthreads();
    const int cols = n - j0 < kTile ? n - j0 : kTile;
    if (row < n) {
      const auto key_of = [&](int c) {
        const float dx = yi[0] - ys[c][0], dy = yi[1] - ys[c][1];
        return knn_key(dx * dx + dy * dy, j0 + c);
      };
      uint64_t mask = 0;
      for (int c = 0; c < cols; ++c) mask |= (uint64_t)(j0 + c != row && key_of(c) < worst) << c;
      knn_take(mask, list, kTile, k, worst, key_of);
    }
  }
  if (row < n)
    for (int s = 0; s < k; ++s) {
      const uint64_t key = list[s * kTile];
      ynbr[(size_t)row * k + s] = key == kEmpty ? -1 : (int32_t)(uint32_t)key;
    }
}

// thr[i][s] = the key (D_ij, j) of row i's s-th map neighbour j; one wave per 32 rows.  Lane (kh, l32) holds row
// i = 32 block + l32 as the A operand and its neighbour's row as the B operand, both in dad_gram_load_a's layout, so
// the block's diagonal entry (l32, l32) is the walk's entry (i, j).
__global__ __launch_bounds__(64) void dad_knn_gather(const float* __restrict__ emb, const float* __restrict__ norms,
                                                     const float* __restrict__ mean, const int32_t* __restrict__ ynbr,
                                                     int n, int k, uint64_t* __restrict__ thr) {
  const int lane = threadIdx.x, kh = lane >> 5, l32 = lane & 31;
  const int ia = 32 * (int)blockIdx.x + l32;
  f32x4 av[DAD_H / 8];
  dad_gram_load_a(av, emb, mean, ia, n, kh);
  const float ni = norms[ia];          // (64 * ceil(n / 64) entries)
  for (int s = 0; s < k; ++s) {
    const int j = ia < n ? ynbr[(size_t)ia * k + s] : -1;
    const bool have = j >= 0 && j < n;
    const float* rb = emb + (size_t)(have ? j : 0) * DAD_H + 4 * kh;
    f32x16 acc = f32x16{};
#pragma unroll 4
    for (int q = 0; q < DAD_H / 8; ++q) {
      const f32x4 bv = have ? *reinterpret_cast<const f32x4*>(rb + 8 * q) -
                                  *reinterpret_cast<const f32x4*>(mean + 4 * kh + 8 * q)
                            : f32x4{};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][e], bv[e], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (l32 == dad_acc_row(r, kh) && ia < n)
        thr[(size_t)ia * k + s] = have ? knn_key(dad_pair_d2(ni, norms[j], acc[r], ia, j), j) : 0ull;
  }
}

struct KnnCountArgs {
  const float* emb;
  const float* norms;
  const float* mean;
  const uint64_t* thr;  // [npad][k]
  int32_t* cpart;       // [chunks][npad][k]
  int n, npad, ct, per, k;
};

template <int KCAP>
__global__ __launch_bounds__(kThreads, KCAP <= 16 ? 2 : 1) void dad_knn_count(KnnCountArgs a) {
  __shared__ __attribute__((aligned(16))) float bt[kTile * kGramLd];
  __shared__ float nj_s[kTile], ni_s[kTile];
  __shared__ uint64_t thr_s[KCAP * kTile];       // [slot][row]
  __shared__ int cnt_s[KCAP * kTile];
  const int tid = threadIdx.x;
  const int i0 = kTile * (int)blockIdx.x, chunk = blockIdx.y, n = a.n, k = a.k;
  for (int e = tid; e < k * kTile; e += kThreads) {
    const int s = e >> 6, row = e & 63;
    thr_s[e] = i0 + row < n ? a.thr[(size_t)(i0 + row) * k + s] : 0ull;    // (nothing is below key 0)
    cnt_s[e] = 0;
  }
  float* dt = bt;
  const int row = tid >> 2, q4 = tid & 3;        // four lanes per row, 16 columns each

  dad_gram_walk_chunk(
      a.emb, a.norms, a.mean, n, i0, chunk, a.per, a.ct, bt, nj_s, ni_s, [](int, int) {},
      [&](int r, int ig, int jc, int jg, float d2) {
        if (r == 0) __syncthreads();       // every wave's operand reads of this tile are done
        dt[(ig - i0) * kDtLd + jc] = d2;
        if (r == 15) {
          __syncthreads();
          const int c0 = jg - jc + 16 * q4, me = i0 + row;
          uint64_t kc[16];
#pragma unroll
          for (int e = 0; e < 16; ++e)
            kc[e] = c0 + e < n && c0 + e != me ? knn_key(dt[row * kDtLd + 16 * q4 + e], c0 + e) : kEmpty;
          for (int s = 0; s < k; ++s) {
            const uint64_t t = thr_s[s * kTile + row];
            const int js = (int)(uint32_t)t;
            int c = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) c += kc[e] < t && c0 + e != js;
            c += __shfl_xor(c, 1, 64);
            c += __shfl_xor(c, 2, 64);
            if (q4 == 0) cnt_s[s * kTile + row] += c;
          }
        }
      });
  __syncthreads();
  for (int e = tid; e < k * kTile; e += kThreads) {
    const int s = e >> 6, rr = e & 63;
    a.cpart[((size_t)chunk * a.npad + i0 + rr) * k + s] = cnt_s[e];
  }
}

__global__ __launch_bounds__(kThreads) void dad_knn_penalty(const int32_t* __restrict__ cpart, int n, int npad,
                                                            int chunks, int k, int32_t* __restrict__ pen,
                                                            int32_t* __restrict__ penalty) {
  const int i = kThreads * (int)blockIdx.x + threadIdx.x;
  if (i >= n) return;
  int p = 0;
  for (int s = 0; s < k; ++s) {
    int c = 0;
    for (int q = 0; q < chunks; ++q) c += cpart[((size_t)q * npad + i) * k + s];
    const int over = 1 + c - k;        // rank - k
    p += over > 0 ? over : 0;
  }
  pen[i] = p;
  if (penalty) penalty[i] = p;
}

__global__ __launch_bounds__(kThreads) void dad_knn_trust(const int32_t* __restrict__ pen, const float* __restrict__ Y,
                                                          const int32_t* __restrict__ hdr, int n, int k,
                                                          double* __restrict__ out) {
  __shared__ long long red[kThreads];
  __shared__ int bad_s[kThreads];
  const int tid = threadIdx.x;
  long long s = 0;
  int bad = 0;
  for (int i = tid; i < n; i += kThreads) {
    s += pen[i];
    bad += nonfinite(Y[2 * i]) | nonfinite(Y[2 * i + 1]);
  }
  red[tid] = s;
  bad_s[tid] = bad;
  __syncthreads();
  if (tid == 0) {
    long long tot = 0;
    int nb = hdr[kHdrBad];
    for (int d = 0; d < kThreads; ++d) {
      tot += red[d];
      nb += bad_s[d];
    }
    const double nd = (double)n, kd = (double)k;
    out[DAD_TW_T] = 1.0 - (double)tot * (2.0 / (nd * kd * (2.0 * nd - 3.0 * kd - 1.0)));
    out[DAD_TW_PENALTY] = (double)tot;
    out[DAD_TW_N] = nd;
    out[DAD_TW_K] = kd;
    out[DAD_TW_VALID] = nb == 0 ? 1.0 : 0.0;
    out[DAD_TW_NONFINITE] = (double)nb;
    out[6] = 0.0;
    out[7] = 0.0;
  }
}

namespace {

int knn_shape(int64_t n, int k) { return n < 1 || n > DAD_KNN_MAX_N || k < 1 || k > kMaxK ? DAD_E_SHAPE : DAD_OK; }

// dad_knn_plan at this k, as pair_resolve's planner
auto knn_planner(int k) {
  return [k](int64_t n, int cus, int* rt, int* ch, int* per) { return dad_knn_plan(n, k, cus, rt, ch, per); };
}

// what every walk of this file starts from: the mean of the rows with group >= 0, their norms, the header
int knn_centre(const float* emb, const int32_t* group, int64_t n, int rt, const KnnWs& L, void* ws, hipStream_t stream) {
  float* mean = ws_ptr<float>(ws, L.mean);
  double* csum = ws_ptr<double>(ws, L.csum);
  int32_t *cnt = ws_ptr<int32_t>(ws, L.cnt), *hdr = ws_ptr<int32_t>(ws, L.hdr);
  return pair_centre<1, false>(emb, PairInt32Group{group}, nullptr, n, rt, csum, cnt, nullptr, mean,
                               ws_ptr<float>(ws, L.norms), stream, [&] {
    hipLaunchKernelGGL(dad_pair_mean, dim3(1), dim3(kThreads), 0, stream, csum, cnt, rt, mean, hdr);
  });
}

}  // namespace

extern "C" int dad_knn_plan(int64_t n, int k, int cus, int* row_tiles, int* chunks, int* tiles_per_chunk) {
  if (!row_tiles || !chunks || !tiles_per_chunk) return DAD_E_ARG;
  if (knn_shape(n, k) || cus < 1) return DAD_E_SHAPE;
  // the most chunks whose grid is still resident at once: two workgroups a CU up to k = 16, one above (the lists' LDS)
  const int rt = (int)((n + kTile - 1) / kTile);
  return pair_plan_out(pair_plan(n, (k <= 16 ? 2 : 1) * cus / rt, kMaxChunks), row_tiles, chunks, tiles_per_chunk);
}

extern "C" size_t dad_knn_workspace_bytes(int64_t n, int k) {
  if (knn_shape(n, k)) return 0;
  return knn_ws_layout(n, k).bytes;
}

extern "C" int dad_knn_chunked(const float* emb, const int32_t* group, int64_t n, int k, int mode, int32_t* idx,
                               float* d2, int chunks, void* ws, void* stream_) {
  if (!emb || !idx || !d2 || !ws) return DAD_E_ARG;
  if (mode != DAD_KNN_ALL && mode != DAD_KNN_SAME && mode != DAD_KNN_OTHER) return DAD_E_ARG;
  DAD_RET(knn_shape(n, k));
  PairPlan pl;
  DAD_RET(pair_resolve(n, chunks, kMaxChunks, knn_planner(k), &pl));
  hipStream_t stream = (hipStream_t)stream_;
  const KnnWs L = knn_ws_layout(n, k);
  DAD_RET(knn_centre(emb, group, n, pl.rt, L, ws, stream));
  KnnPairArgs pa;
  pa.emb = emb; pa.group = group; pa.norms = ws_ptr<float>(ws, L.norms); pa.mean = ws_ptr<float>(ws, L.mean);
  pa.part = ws_ptr<uint64_t>(ws, L.keys);
  pa.n = (int)n; pa.npad = pl.rt * kTile; pa.ct = pl.rt; pa.per = pl.per; pa.k = k; pa.mode = mode;
  if (k <= 16) hipLaunchKernelGGL(dad_knn_pair<16>, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, pa);
  else hipLaunchKernelGGL(dad_knn_pair<kMaxK>, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, pa);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_knn_merge, dim3(pl.rt), dim3(kTile), 0, stream, pa.part, (int)n, pa.npad, pl.chunks, k, idx, d2);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_knn(const float* emb, const int32_t* group, int64_t n, int k, int mode, int32_t* idx, float* d2,
                       void* workspace, void* stream) {
  return dad_knn_chunked(emb, group, n, k, mode, idx, d2, 0, workspace, stream);
}

extern "C" int dad_knn_vote(const int32_t* idx, const int64_t* labels, const int32_t* group, int64_t n, int k,
                            int64_t* pred, int64_t* out, void* stream_) {
  if (!idx || !labels || !pred || !out) return DAD_E_ARG;
  DAD_RET(knn_shape(n, k));
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(dad_knn_vote_clear, dim3(1), dim3(64), 0, stream, reinterpret_cast<unsigned long long*>(out));
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_knn_vote_rows, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, idx,
                     labels, group, (int)n, k, pred, reinterpret_cast<unsigned long long*>(out));
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_trustworthiness_chunked(const float* emb, const float* Y, int64_t n, int k, double* out,
                                           int32_t* penalty, int chunks, void* ws, void* stream_) {
  if (!emb || !Y || !out || !ws) return DAD_E_ARG;
  DAD_RET(knn_shape(n, k));
  if (2 * (int64_t)k >= n) return DAD_E_SHAPE;     // scikit-learn: n_neighbors < n_samples / 2
  PairPlan pl;
  DAD_RET(pair_resolve(n, chunks, kMaxChunks, knn_planner(k), &pl));
  hipStream_t stream = (hipStream_t)stream_;
  const KnnWs L = knn_ws_layout(n, k);
  DAD_RET(knn_centre(emb, nullptr, n, pl.rt, L, ws, stream));
  int32_t *ynbr = ws_ptr<int32_t>(ws, L.ynbr), *pen = ws_ptr<int32_t>(ws, L.pen);
  uint64_t* thr = ws_ptr<uint64_t>(ws, L.thr);
  hipLaunchKernelGGL(dad_knn_y, dim3(pl.rt), dim3(kTile), 0, stream, Y, (int)n, k, ynbr);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_knn_gather, dim3(2 * pl.rt), dim3(64), 0, stream, emb, ws_ptr<float>(ws, L.norms),
                     ws_ptr<float>(ws, L.mean), ynbr, (int)n, k, thr);
  DAD_TRY(hipGetLastError());
  KnnCountArgs ca;
  ca.emb = emb; ca.norms = ws_ptr<float>(ws, L.norms); ca.mean = ws_ptr<float>(ws, L.mean); ca.thr = thr;
  ca.cpart = ws_ptr<int32_t>(ws, L.keys);
  ca.n = (int)n; ca.npad = pl.rt * kTile; ca.ct = pl.rt; ca.per = pl.per; ca.k = k;
  if (k <= 16) hipLaunchKernelGGL(dad_knn_count<16>, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, ca);
  else hipLaunchKernelGGL(dad_knn_count<kMaxK>, dim3(pl.rt, pl.chunks), dim3(kThreads), 0, stream, ca);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_knn_penalty, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                     ca.cpart, (int)n, ca.npad, pl.chunks, k, pen, penalty);
  DAD_TRY(hipGetLastError());
  hipLaunchKernelGGL(dad_knn_trust, dim3(1), dim3(kThreads), 0, stream, pen, Y, ws_ptr<int32_t>(ws, L.hdr), (int)n, k,
                     out);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

extern "C" int dad_trustworthiness(const float* emb, const float* Y, int64_t n, int k, double* out, int32_t* penalty,
                                   void* workspace, void* stream) {
  return dad_trustworthiness_chunked(emb, Y, n, k, out, penalty, 0, workspace, stream);
}
