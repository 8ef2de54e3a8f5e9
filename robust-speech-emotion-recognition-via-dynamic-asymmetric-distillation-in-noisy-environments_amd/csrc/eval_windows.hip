// Emotion over time, store-fed: one call classifies every sliding window or every prefix of every utterance
// of a FeatureStore split, in one pass over the store (dad.h, "windows of a split").
//
// The encoder is frame-wise, so the embedding of frames [a, b) is a partial sum of the per-frame rows
// relu(W1 x_t + b1) that dad_eval_encode (eval_split.hip) computes and sums per slab.  Here the same GEMM's
// epilogue sums them per PIECE: a maximal run of frames inside one 32-frame slab and one hop-segment
// [s hop, (s + 1) hop).  An utterance's pieces, in frame order, are cut at every multiple of 32 and of hop
// below its length; a window is a run of whole pieces.
//
// Four launches, no host work in between:
//   dad_window_encode   dad_eval_encode's work unit (one wave = one 32-frame slab x all 256 hidden units, rows
//                       read in place, eval_rows.h's loaders / GEMM loop); the slab epilogue runs once per piece
//                       with the piece's row mask -> piece[P][256].  A slab holds at most
//                       min(32, ceil(32 / hop) + 1) pieces, so hop >= 32 costs at most two epilogues a slab.
//                       hop = 1 (a piece is a frame) stores every lane's own rows instead: rows_epilogue.
//   dad_window_head_*   a window's sum is the left-to-right fp32 sum of its pieces in frame order, from 0, as
//                       dad_eval_head sums slab partials.  PREFIX: one wave per utterance keeps the running sum
//                       and emits a window at every segment end (O(len)).  SLIDING: one wave per window re-sums
//                       its pieces (no subtraction of running sums: exact, independent of j).  Then
//                       eval_head_pooled: / frames, classifier, softmax, score, first-maximum argmax.
//   dad_window_utt      one thread per utterance: mean probabilities, vote, last, settle, switches.
//   dad_window_result   one workgroup: the DAD_EW_* block (integer LDS atomics).
// No floating-point atomics anywhere: two calls on the same inputs write the same bits.  For hop % 32 == 0 a
// piece is a slab, so PREFIX's last window repeats dad_eval_split's arithmetic exactly.
#include <cstring>

#include "dad_common.h"
#include "dad_kernels.h"
#include "eval_rows.h"

namespace {

constexpr int kEncThreads = 256;     // 4 waves, one slab each
constexpr int kHeadWaves = 4;
constexpr int kUttThreads = 256;
constexpr int kResThreads = 256;
static_assert(kResThreads == DAD_EW_SLOTS && kResThreads == 4 * DAD_EW_CURVE, "dad_window_result's thread roles");

struct WinGeom {
  int hop, span, mode;
  long long lcm;                     // lcm(32, hop)
};

struct WinEncArgs {
  const void* store;
  const int64_t* rows; const int32_t* lens; const int32_t* slab_off; const int32_t* piece_off;
  int n, slabs, pieces;
  WinGeom g;
  const float* params;               // flat [W1|b1|W2|b2]
  const uint16_t* w1h;               // FP16: row-major fp16 W1 copy
  float* piece;                      // [pieces][256]
};

struct WinHeadArgs {
  int n, windows, pieces, use_entropy;
  WinGeom g;
  const int32_t* lens; const int32_t* win_off; const int32_t* piece_off;
  const float* piece; const float* params;
  float* w_emb; float* w_logits; float* probs; float* w_score; int64_t* w_pred;   // probs: w_probs or the workspace
  int32_t* ws_pred; int32_t* ws_bad;
};

struct WinUttArgs {
  int n, windows;
  WinGeom g;
  const int32_t* lens; const int32_t* win_off;
  const float* probs; const int32_t* ws_pred;
  float* mean_probs; int64_t* mean_pred; int64_t* vote_pred; int64_t* last_pred; int32_t* settle; int32_t* switches;
  int32_t* u_J; int32_t* u_mean; int32_t* u_vote; int32_t* u_last; int32_t* u_settle; int32_t* u_switches;
  int32_t* u_frames;
};

struct WinResArgs {
  int n, windows;
  const int64_t* labels; const int32_t* win_off;
  const int32_t* ws_pred; const int32_t* ws_bad;
  const int32_t* u_J; const int32_t* u_mean; const int32_t* u_vote; const int32_t* u_last; const int32_t* u_settle;
  const int32_t* u_switches; const int32_t* u_frames;
  int64_t* result;
};

// windows of an utterance of len frames (dad.h's definitions)
__device__ __forceinline__ int win_count(int len, const WinGeom& g) {
  if (len <= 0) return 0;
  const int S = (len - 1) / g.hop + 1;
  if (g.mode == DAD_WIN_PREFIX) return S;
  const long long J = (long long)S - g.span + 1;
  return J < 1 ? 1 : (int)J;
}

// the utterance's pieces that start before frame x: the multiples of 32 or of hop in [0, x)
__device__ __forceinline__ long long pieces_before(long long x, const WinGeom& g) {
  return (x + 31) / 32 + (x + g.hop - 1) / g.hop - (x + g.lcm - 1) / g.lcm;
}

// window count of utterance u if its win_off entries agree with its length and lie inside [0, windows], else 0
__device__ __forceinline__ int win_range(const int32_t* lens, const int32_t* win_off, int windows, int u,
                                         const WinGeom& g, int* w0) {
  const int J = win_count(lens[u], g);
  const int a = win_off[u], b = win_off[u + 1];
  *w0 = a;
  return (a >= 0 && b <= windows && b - a == J) ? J : 0;
}

// hop = 1: every frame is its own piece.  eval_epilogue under a one-row mask returns the row itself (0 + x in the
// lane that holds the row, + 0 from the other lane half), so each lane stores the ReLU of its own 16 rows: the same
// bits as thirty-two masked passes, at the cost of one.  Row k of the slab is piece first + k.
__device__ __forceinline__ void rows_epilogue(const f32x16* acc, const float* bias, float* piece, long long first,
                                              long long pieces, uint32_t vbits) {
  const int lane = threadIdx.x & 63;
  const int j = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    const float bh = bias[ht * 32 + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = dad_acc_row(r, kh);
      const float pre = acc[ht][r] + bh;
      if (((vbits >> row) & 1u) && first + row < pieces)
        piece[(size_t)(first + row) * DAD_H + ht * 32 + j] = !(pre <= 0.0f) ? pre : 0.0f;   // (keeps a NaN)
    }
  }
}

template <int DT, bool F16>
__global__ __launch_bounds__(kEncThreads) void dad_window_encode(WinEncArgs a) {
  DAD_GUARD_BLOCK(kEncThreads);
  const int lane = threadIdx.x & 63;
  const int job = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kEncThreads / 64) + (threadIdx.x >> 6)));
  if (job >= a.slabs) return;
  const int u = slab_owner(a.slab_off, a.n, job);
  const int len = a.lens[u];
  const int c = job - a.slab_off[u];
  const int i = lane & 31, kh = lane >> 5;
  const int t = c * DAD_SLAB + i;
  const uint32_t vbits = (uint32_t)__ballot(t < len && c >= 0);
  if (vbits == 0u) return;           // a table that disagrees with lens: nothing read, nothing written
  f32x16 acc0[DAD_HT], acc1[DAD_HT];
#pragma unroll
  for (int ht = 0; ht < DAD_HT; ++ht) {
    acc0[ht] = f32x16{};
    acc1[ht] = f32x16{};
  }
  // past the last frame: the utterance's last row again (no piece's mask holds it)
  const size_t row = (size_t)(a.rows[u] + (int64_t)min(t, len - 1));
  if constexpr (F16) {
    eval_slab_f16<DT, false>(a.store, row * DAD_D + 8 * kh, a.w1h + (size_t)i * DAD_D + 8 * kh, nullptr, acc0, acc1);
  } else {
    eval_slab_f32<DT, false>(a.store, row * DAD_D + 4 * kh, a.params + DAD_OFF_W1 + (size_t)i * DAD_D + 4 * kh, nullptr,
                             acc0, acc1);
  }
  // the slab's valid frames [t0, t1) cut at the multiples of hop
  const int t0 = c * DAD_SLAB;
  const int t1 = min(len - t0, DAD_SLAB) + t0;
  long long idx = (long long)a.piece_off[u] + pieces_before(t0, a.g);
  if (idx < 0) return;
  if (a.g.hop == 1) {
    rows_epilogue(acc0, a.params + DAD_OFF_B1, a.piece, idx, (long long)a.pieces, vbits);
    return;
  }
  for (int s = t0; s < t1; ++idx) {
    const int nrow = min(a.g.hop - s % a.g.hop, t1 - s);                     // 1 .. 32
    const uint32_t mask = (nrow >= 32 ? 0xffffffffu : (1u << nrow) - 1u) << (s - t0);
    if (idx < (long long)a.pieces) eval_epilogue(acc0, a.params + DAD_OFF_B1, a.piece + (size_t)idx * DAD_H, mask);
    s += nrow;
  }
}

// row-major fp16 copy of the network's W1
__global__ __launch_bounds__(256) void dad_window_w1h(const float* params, uint16_t* w) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)DAD_H * DAD_D) return;
  w[i] = dad_half_bits(params[DAD_OFF_W1 + i], true);
}

// window w = the pooled sum s over `frames` frames: outputs and the workspace's prediction / non-finite flag
__device__ __forceinline__ void window_emit(const WinHeadArgs& a, int w, f32x4 s, int frames) {
  bool bad = false;
  const int am = eval_head_pooled(s, (float)frames, a.params, a.use_entropy, (size_t)w, a.w_emb, a.w_logits, a.probs,
                                  a.w_score, nullptr, &bad);
  if ((threadIdx.x & 63) == 0) {
    if (a.w_pred) a.w_pred[w] = am;
    a.ws_pred[w] = am;
    a.ws_bad[w] = bad ? 1 : 0;
  }
}

// SLIDING: one wave per window
__global__ __launch_bounds__(64 * kHeadWaves) void dad_window_head_sliding(WinHeadArgs a) {
  DAD_GUARD_BLOCK(64 * kHeadWaves);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kHeadWaves + (threadIdx.x >> 6)));
  if (w >= a.windows) return;
  const int u = slab_owner(a.win_off, a.n, w);
  int w0;
  const int J = win_range(a.lens, a.win_off, a.windows, u, a.g, &w0);
  const int j = w - w0;
  if (j < 0 || j >= J) return;       // inconsistent table
  const int len = a.lens[u];
  const long long f0 = (long long)j * a.g.hop;
  long long f1 = ((long long)j + a.g.span) * a.g.hop;
  if (f1 > len) f1 = len;
  const long long base = a.piece_off[u];
  const long long p0 = base + pieces_before(f0, a.g), p1 = base + pieces_before(f1, a.g);
  if (base < 0 || p1 > (long long)a.pieces) return;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long p = p0; p < p1; ++p) s += *reinterpret_cast<const f32x4*>(a.piece + (size_t)p * DAD_H + 4 * lane);
  window_emit(a, w, s, (int)(f1 - f0));
}

// PREFIX: one wave per utterance, a running sum over its pieces, a window at every segment end
__global__ __launch_bounds__(64 * kHeadWaves) void dad_window_head_prefix(WinHeadArgs a) {
  DAD_GUARD_BLOCK(64 * kHeadWaves);
  const int lane = threadIdx.x & 63;
  const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kHeadWaves + (threadIdx.x >> 6)));
  if (u >= a.n) return;
  int w0;
  const int J = win_range(a.lens, a.win_off, a.windows, u, a.g, &w0);
  if (J == 0) return;
  const int len = a.lens[u];
  long long p = a.piece_off[u];
  if (p < 0 || p + pieces_before(len, a.g) > (long long)a.pieces) return;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  int cur = 0, j = 0;
  while (cur < len && j < J) {
    const int step = min(min(DAD_SLAB - (cur & (DAD_SLAB - 1)), a.g.hop - cur % a.g.hop), len - cur);
    s += *reinterpret_cast<const f32x4*>(a.piece + (size_t)p * DAD_H + 4 * lane);
    ++p;
    cur += step;
    if (cur % a.g.hop == 0 || cur == len) {
      window_emit(a, w0 + j, s, cur);
      ++j;
    }
  }
}

__global__ __launch_bounds__(kUttThreads) void dad_window_utt(WinUttArgs a) {
  DAD_GUARD_BLOCK(kUttThreads);
  const int u = (int)(blockIdx.x * kUttThreads + threadIdx.x);
  if (u >= a.n) return;
  int w0;
  const int J = win_range(a.lens, a.win_off, a.windows, u, a.g, &w0);
  float ps[DAD_C] = {0.f, 0.f, 0.f, 0.f};
  int votes[DAD_C] = {0, 0, 0, 0};
  int mean = -1, vote = -1, last = -1, settle = -1, switches = -1, frames = 0;
  if (J > 0) {
    settle = 0;
    switches = 0;
    for (int j = 0; j < J; ++j) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(a.probs + (size_t)(w0 + j) * DAD_C);
      const int pr = a.ws_pred[w0 + j];
#pragma unroll
      for (int c = 0; c < DAD_C; ++c) {
        ps[c] += p[c];
        votes[c] += pr == c ? 1 : 0;
      }
      if (j >= 1 && pr != last) { ++switches; settle = j; }
      last = pr;
    }
    mean = 0;
    vote = 0;
#pragma unroll
    for (int c = 0; c < DAD_C; ++c) ps[c] = ps[c] / (float)J;
#pragma unroll
    for (int c = 1; c < DAD_C; ++c) {
      if (ps[c] > ps[mean]) mean = c;
      if (votes[c] > votes[vote]) vote = c;
    }
    const int len = a.lens[u];
    const long long e = ((long long)settle + (a.g.mode == DAD_WIN_PREFIX ? 1 : a.g.span)) * a.g.hop;
    frames = e < len ? (int)e : len;
  }
  if (a.mean_probs) *reinterpret_cast<f32x4*>(a.mean_probs + (size_t)u * DAD_C) = f32x4{ps[0], ps[1], ps[2], ps[3]};
  if (a.mean_pred) a.mean_pred[u] = mean;
  if (a.vote_pred) a.vote_pred[u] = vote;
  if (a.last_pred) a.last_pred[u] = last;
  if (a.settle) a.settle[u] = settle;
  if (a.switches) a.switches[u] = switches;
  a.u_J[u] = J; a.u_mean[u] = mean; a.u_vote[u] = vote; a.u_last[u] = last;
  a.u_settle[u] = settle; a.u_switches[u] = switches; a.u_frames[u] = frames;
}

__global__ __launch_bounds__(kResThreads) void dad_window_result(WinResArgs a) {
  DAD_GUARD_BLOCK(kResThreads);
  __shared__ unsigned long long cnt[DAD_EW_SLOTS];
  const int tid = threadIdx.x;
  cnt[tid] = 0ull;
  __syncthreads();
  for (int u = tid; u < a.n; u += kResThreads) {
    const long y = a.labels ? (long)a.labels[u] : -1;
    const bool lab = y >= 0 && y < DAD_C;
    const int J = a.u_J[u];
    if (lab) atomicAdd(&cnt[DAD_EW_N_LABELLED], 1ull);
    if (J == 0) {
      atomicAdd(&cnt[DAD_EW_N_EMPTY], 1ull);
      continue;
    }
    if (lab) {
      atomicAdd(&cnt[DAD_EW_CONF_MEAN + (int)y * DAD_C + a.u_mean[u]], 1ull);
      atomicAdd(&cnt[DAD_EW_CONF_VOTE + (int)y * DAD_C + a.u_vote[u]], 1ull);
      atomicAdd(&cnt[DAD_EW_CONF_LAST + (int)y * DAD_C + a.u_last[u]], 1ull);
    }
    atomicAdd(&cnt[DAD_EW_SETTLE_SUM], (unsigned long long)a.u_settle[u]);
    atomicAdd(&cnt[DAD_EW_SWITCHES_SUM], (unsigned long long)a.u_switches[u]);
    atomicAdd(&cnt[DAD_EW_SETTLE_FRAMES_SUM], (unsigned long long)a.u_frames[u]);
  }
  unsigned long long nbad = 0ull;
  for (int w = tid; w < a.windows; w += kResThreads) nbad += a.ws_bad[w] ? 1ull : 0ull;
  atomicAdd(&cnt[DAD_EW_N_NONFINITE], nbad);
  // the curve: thread (j, g) counts slot j over the utterances g, g + 4, ... in registers
  {
    const int j = tid & (DAD_EW_CURVE - 1), g = tid / DAD_EW_CURVE;
    unsigned long long reached = 0ull, correct = 0ull, carried = 0ull;
    for (int u = g; u < a.n; u += kResThreads / DAD_EW_CURVE) {
      const long y = a.labels ? (long)a.labels[u] : -1;
      const int J = a.u_J[u];
      if (y < 0 || y >= DAD_C || J == 0) continue;
      const int w0 = a.win_off[u];
      const bool hit = a.ws_pred[w0 + min(j, J - 1)] == (int)y;
      carried += hit ? 1ull : 0ull;
      if (J > j) {
        ++reached;
        correct += hit ? 1ull : 0ull;
      }
    }
    atomicAdd(&cnt[DAD_EW_REACHED + j], reached);
    atomicAdd(&cnt[DAD_EW_CORRECT + j], correct);
    atomicAdd(&cnt[DAD_EW_CARRIED + j], carried);
  }
  __syncthreads();
  int64_t v = (int64_t)cnt[tid];
  if (tid == DAD_EW_N) v = a.n;
  if (tid == DAD_EW_N_WINDOWS) v = a.windows;
  a.result[tid] = v;
}

struct WinWs {
  size_t piece, pred, bad, probs, utt, w1h, bytes;
};

WinWs win_ws_layout(int64_t n, int64_t windows, int64_t pieces, int precision) {
  WinWs w;
  size_t off = 0;
  const size_t np = (size_t)(pieces > 0 ? pieces : 1), nw = (size_t)(windows > 0 ? windows : 1);
  w.piece = off; off = dad_align(off + sizeof(float) * np * DAD_H);
  w.pred = off;  off = dad_align(off + sizeof(int32_t) * nw);
  w.bad = off;   off = dad_align(off + sizeof(int32_t) * nw);
  w.probs = off; off = dad_align(off + sizeof(float) * nw * DAD_C);
  w.utt = off;   off = dad_align(off + sizeof(int32_t) * 7 * (size_t)n);
  w.w1h = off;   off = dad_align(off + (precision == DAD_PREC_FP16 ? sizeof(uint16_t) * DAD_H * DAD_D : 0));
  w.bytes = off;
  return w;
}

bool win_shape_ok(int64_t n, int64_t slabs, int64_t windows, int64_t pieces) {
  return n >= 1 && n <= 0x7fffffffLL && slabs >= 0 && slabs <= 0x7fffffffLL && slabs <= n * (int64_t)(1 << 26) &&
         windows >= 0 && windows <= 0x7fffffffLL && pieces >= slabs && pieces <= 0x7fffffffLL;
}

template <int DT>
void launch_encode(const WinEncArgs& ea, bool f16, hipStream_t stream) {
  const dim3 grid((unsigned)((ea.slabs + kEncThreads / 64 - 1) / (kEncThreads / 64))), block(kEncThreads);
  if (f16) hipLaunchKernelGGL((dad_window_encode<DT, true>), grid, block, 0, stream, ea);
  else hipLaunchKernelGGL((dad_window_encode<DT, false>), grid, block, 0, stream, ea);
}

}  // namespace

extern "C" size_t dad_eval_windows_workspace_bytes(int64_t n, int64_t slabs, int64_t windows, int64_t pieces,
                                                   int precision) {
  if (!win_shape_ok(n, slabs, windows, pieces)) return 0;
  return win_ws_layout(n, windows, pieces, precision).bytes;
}

extern "C" int dad_eval_windows(const dad_window_args* args, void* workspace, void* stream_) {
  if (!args || !workspace) return DAD_E_ARG;
  if (!args->store || !args->rows || !args->lens || !args->slab_off || !args->params || !args->win_off ||
      !args->piece_off || !args->win_off_host || !args->result)
    return DAD_E_ARG;
  const int dt = args->store_dtype;
  if (dt != DAD_STORE_F32 && dt != DAD_STORE_F16 && dt != DAD_STORE_BF16) return DAD_E_ARG;
  if (args->hop < 1 || args->span < 1) return DAD_E_ARG;
  if (args->mode != DAD_WIN_SLIDING && args->mode != DAD_WIN_PREFIX) return DAD_E_ARG;
  if (args->mode == DAD_WIN_PREFIX && args->span != 1) return DAD_E_ARG;
  if (args->precision == DAD_PREC_BF16) return DAD_E_UNSUPPORTED;
  if (args->precision != DAD_PREC_FP32 && args->precision != DAD_PREC_FP16) return DAD_E_ARG;
  if (!win_shape_ok(args->n, args->slabs, args->windows, args->pieces)) return DAD_E_SHAPE;
  if (args->win_off_host[0] != 0 || (int64_t)args->win_off_host[args->n] != args->windows) return DAD_E_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const bool f16 = args->precision == DAD_PREC_FP16;
  const WinWs L = win_ws_layout(args->n, args->windows, args->pieces, args->precision);
  char* ws = (char*)workspace;
  const int n = (int)args->n;

  WinGeom g;
  g.hop = args->hop; g.span = args->span; g.mode = args->mode;
  int two = 1;                       // gcd(32, hop)
  while (two < 32 && args->hop % (2 * two) == 0) two *= 2;
  g.lcm = (long long)args->hop * (32 / two);

  WinEncArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.store = args->store; ea.rows = args->rows; ea.lens = args->lens; ea.slab_off = args->slab_off;
  ea.piece_off = args->piece_off;
  ea.n = n; ea.slabs = (int)args->slabs; ea.pieces = (int)args->pieces;
  ea.g = g;
  ea.params = args->params;
  ea.w1h = (const uint16_t*)(ws + L.w1h);
  ea.piece = (float*)(ws + L.piece);
  if (ea.slabs > 0) {
    if (f16) {
      hipLaunchKernelGGL(dad_window_w1h, dim3((DAD_H * DAD_D + 255) / 256), dim3(256), 0, stream, args->params,
                         (uint16_t*)(ws + L.w1h));
      DAD_TRY(hipGetLastError());
    }
    switch (dt) {
      case DAD_STORE_F16: launch_encode<DAD_STORE_F16>(ea, f16, stream); break;
      case DAD_STORE_BF16: launch_encode<DAD_STORE_BF16>(ea, f16, stream); break;
      default: launch_encode<DAD_STORE_F32>(ea, f16, stream); break;
    }
    DAD_TRY(hipGetLastError());
  }

  WinHeadArgs ha;
  memset(&ha, 0, sizeof(ha));
  ha.n = n; ha.windows = (int)args->windows; ha.pieces = ea.pieces; ha.use_entropy = args->use_entropy;
  ha.g = g;
  ha.lens = args->lens; ha.win_off = args->win_off; ha.piece_off = args->piece_off;
  ha.piece = ea.piece; ha.params = args->params;
  ha.w_emb = args->w_emb; ha.w_logits = args->w_logits; ha.w_score = args->w_score; ha.w_pred = args->w_pred;
  ha.probs = args->w_probs ? args->w_probs : (float*)(ws + L.probs);
  ha.ws_pred = (int32_t*)(ws + L.pred); ha.ws_bad = (int32_t*)(ws + L.bad);
  if (ha.windows > 0) {
    if (g.mode == DAD_WIN_PREFIX)
      hipLaunchKernelGGL(dad_window_head_prefix, dim3((unsigned)((n + kHeadWaves - 1) / kHeadWaves)),
                         dim3(64 * kHeadWaves), 0, stream, ha);
    else
      hipLaunchKernelGGL(dad_window_head_sliding, dim3((unsigned)((ha.windows + kHeadWaves - 1) / kHeadWaves)),
                         dim3(64 * kHeadWaves), 0, stream, ha);
    DAD_TRY(hipGetLastError());
  }

  WinUttArgs ua;
  memset(&ua, 0, sizeof(ua));
  ua.n = n; ua.windows = ha.windows; ua.g = g;
  ua.lens = args->lens; ua.win_off = args->win_off;
  ua.probs = ha.probs; ua.ws_pred = ha.ws_pred;
  ua.mean_probs = args->mean_probs; ua.mean_pred = args->mean_pred; ua.vote_pred = args->vote_pred;
  ua.last_pred = args->last_pred; ua.settle = args->settle; ua.switches = args->switches;
  int32_t* ub = (int32_t*)(ws + L.utt);
  ua.u_J = ub; ua.u_mean = ub + (size_t)n; ua.u_vote = ub + 2 * (size_t)n; ua.u_last = ub + 3 * (size_t)n;
  ua.u_settle = ub + 4 * (size_t)n; ua.u_switches = ub + 5 * (size_t)n; ua.u_frames = ub + 6 * (size_t)n;
  hipLaunchKernelGGL(dad_window_utt, dim3((unsigned)((n + kUttThreads - 1) / kUttThreads)), dim3(kUttThreads), 0, stream,
                     ua);
  DAD_TRY(hipGetLastError());

  WinResArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.n = n; ra.windows = ha.windows; ra.labels = args->labels; ra.win_off = args->win_off;
  ra.ws_pred = ha.ws_pred; ra.ws_bad = ha.ws_bad;
  ra.u_J = ua.u_J; ra.u_mean = ua.u_mean; ra.u_vote = ua.u_vote; ra.u_last = ua.u_last; ra.u_settle = ua.u_settle;
  ra.u_switches = ua.u_switches; ra.u_frames = ua.u_frames;
  ra.result = args->result;
  hipLaunchKernelGGL(dad_window_result, dim3(1), dim3(kResThreads), 0, stream, ra);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}
