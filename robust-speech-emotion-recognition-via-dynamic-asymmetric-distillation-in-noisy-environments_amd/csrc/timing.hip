// Per-kernel timing of the fused step (dad_timing_start / dad_timing_stop): every `every`-th
// step (counted at its encoder call) records hip events at the kernel boundaries of the
// caller's stream.  Events are created up front by dad_timing_start, so a timed region only
// records them.  Not for graph capture.
#include <algorithm>
#include <mutex>
#include <vector>

#include "dad_timing.h"

namespace {

// (event-pair points of each DAD_TK_* kernel: dad_timing_stop's pairs)
const int kTkPairs[DAD_TK_KERNELS][2] = {{TK_E0, TK_E1}, {TK_E1, TK_POOL}, {TK_POOL, TK_TAIL}, {TK_TAIL, TK_WGRAD},
                                         {TK_WGRAD, TK_RED}, {TK_OPT0, TK_OPT1}};
struct Timing {
  unsigned points = ~0u;               // TK points recorded (dad_timing_kernels)
  int every = 0;
  long calls = 0;
  int cur = -1;                        // event set of the step being timed, -1: none
  std::vector<hipEvent_t> ev;          // nset * TK_N
  std::vector<uint8_t> rec;            // recorded flags
  int nset = 0, used = 0;
};
Timing g_tk;
std::mutex g_tk_mu;

}  // namespace

void tk_begin() {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  g_tk.cur = -1;
  if (g_tk.every <= 0) return;
  if (g_tk.calls++ % g_tk.every == g_tk.every - 1 && g_tk.used < g_tk.nset) g_tk.cur = g_tk.used++;
}
void tk_mark(int point, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  if (g_tk.cur < 0 || !((g_tk.points >> point) & 1u)) return;
  const size_t i = (size_t)g_tk.cur * TK_N + point;
  if (hipEventRecord(g_tk.ev[i], s) == hipSuccess) g_tk.rec[i] = 1;
}
void tk_end() {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  g_tk.cur = -1;
}

extern "C" {

int dad_timing_reset(void) {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  if (g_tk.nset <= 0) return DAD_E_ARG;   // no active session
  g_tk.calls = 0;
  g_tk.used = 0;
  g_tk.cur = -1;
  std::fill(g_tk.rec.begin(), g_tk.rec.end(), (uint8_t)0);
  return DAD_OK;
}

int dad_timing_start(int every, int max_steps) {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  if (every < 1 || max_steps < 1) return DAD_E_ARG;
  if (g_tk.nset > 0) return DAD_E_ARG;   // a session is active: dad_timing_stop it first
  for (hipEvent_t e : g_tk.ev) (void)hipEventDestroy(e);
  g_tk = Timing();
  g_tk.ev.assign((size_t)max_steps * TK_N, nullptr);
  g_tk.rec.assign((size_t)max_steps * TK_N, 0);
  // on any failure: the events created so far are destroyed and no session is left half set up
  auto fail = [](hipError_t e, hipStream_t s) {
    for (hipEvent_t x : g_tk.ev)
      if (x) (void)hipEventDestroy(x);
    if (s) (void)hipStreamDestroy(s);
    g_tk = Timing();
    return (int)e;
  };
  // timing-only events: no system-scope fence (no L2 writeback / invalidate at each record, which had
  // cost the stream ~3 us per event and slowed the kernel after it); dad_timing_stop reads them after
  // a device synchronize
  for (auto& e : g_tk.ev) {
    const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    if (r != hipSuccess) return fail(r, nullptr);
  }
  // first use outside the timed region: a HIP event's first record sets it up (host time the
  // first recorded steps would otherwise pay).  Recorded on a private non-blocking stream and
  // synchronised there only: no other stream waits, and a stream capturing a graph is untouched.
  hipStream_t ws = nullptr;
  hipError_t r = hipStreamCreateWithFlags(&ws, hipStreamNonBlocking);
  if (r != hipSuccess) return fail(r, nullptr);
  for (auto& e : g_tk.ev)
    if ((r = hipEventRecord(e, ws)) != hipSuccess) return fail(r, ws);
  if ((r = hipStreamSynchronize(ws)) != hipSuccess) return fail(r, ws);
  (void)hipStreamDestroy(ws);
  g_tk.every = every;
  g_tk.nset = max_steps;
  return DAD_OK;
}

int dad_timing_kernels(unsigned mask) {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  unsigned pts = 0;
  for (int k = 0; k < DAD_TK_KERNELS; ++k)
    if ((mask >> k) & 1u) pts |= (1u << kTkPairs[k][0]) | (1u << kTkPairs[k][1]);
  if (pts & (1u << TK_POOL)) pts |= 1u << TK_E1;   // the tail's start when pooling is fused into it
  g_tk.points = pts;
  return DAD_OK;
}

int dad_timing_stop(double* ms_sum, int* count, int n) {
  std::lock_guard<std::mutex> lk(g_tk_mu);
  const auto& pairs = kTkPairs;
  if (n < 0 || (n > 0 && (!ms_sum || !count))) return DAD_E_ARG;
  for (int k = 0; k < n; ++k) { ms_sum[k] = 0.0; count[k] = 0; }
  int rc = DAD_OK;
  for (int s = 0; s < g_tk.used && rc == DAD_OK; ++s) {
    const size_t b = (size_t)s * TK_N;
    for (int k = 0; k < n && k < DAD_TK_KERNELS; ++k) {
      int a = pairs[k][0];
      const int z = pairs[k][1];
      // pooling fused into the tail launch: no pool point; the tail launch runs from the encoder's end
      if (a == TK_POOL && !g_tk.rec[b + a] && z != TK_POOL) a = TK_E1;
      if (!g_tk.rec[b + a] || !g_tk.rec[b + z]) continue;
      float ms = 0.0f;
      hipError_t e = hipEventSynchronize(g_tk.ev[b + z]);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_tk.ev[b + a], g_tk.ev[b + z]);
      if (e != hipSuccess) { rc = (int)e; break; }
      ms_sum[k] += ms;
      count[k] += 1;
    }
  }
  for (hipEvent_t e : g_tk.ev) (void)hipEventDestroy(e);
  g_tk = Timing();
  return rc;
}

}  // extern "C"
