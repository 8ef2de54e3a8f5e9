// The confirmation-bias log of Trainer.train_step, appended on the device.
//
// Replaces, per step, the reference's host loop over the noisy batch (I/train.py:425-437):
//   batch_indices = noisy_batch['id'].cpu().numpy()
//   for i, sample_idx in enumerate(batch_indices):
//       if int(sample_idx) in self.tracked_sample_indices:
//           self.bias_analysis_log.append({'epoch', 'sample_id', 'pseudo_label': preds[i].item(),
//                                          'certainty_score': certainty_scores[i].item(), 'is_masked_in': mask[i].item()})
// which costs a device->host copy of the ids and three .item() syncs per tracked row.  Here the step's tail
// buffer already holds score / pred / mask of every noisy row; one small launch compacts the tracked rows,
// in batch order, behind the records already in the trace buffer.  The size of the compaction never reaches
// the host: the cursor lives in the buffer's header.
//
// Work: one workgroup, one row per lane (Bn <= DAD_MAX_BATCH = 1024 = 16 waves).  Each lane loads its id and,
// for an id inside [0, n_samples), its bitmap word; a wave-wide ballot and the count of set lanes below the lane
// rank the hits inside the wave, the waves' totals cross through LDS (one barrier), and each record leaves as
// one 16-byte store.  Latency-bound: ~Bn * 20 B read, 16 B per record written.  No atomics: appends to one
// trace are ordered on one stream, so the cursor is read at entry and written once at exit.
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/dad.h"

namespace {

constexpr int kMaxWaves = DAD_MAX_BATCH / 64;
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

static_assert(DAD_TRACE_HDR_WORDS == 4 && DAD_TRACE_REC_WORDS == 4, "records are 16-byte aligned i32x4 stores");

}  // namespace

__global__ __launch_bounds__(DAD_MAX_BATCH) void dad_trace_append_kernel(const float* __restrict__ tail, int Bn,
                                                                         const int64_t* __restrict__ ids,
                                                                         const uint32_t* __restrict__ tracked,
                                                                         long n_samples, int epoch, int32_t* trace,
                                                                         long capacity) {
  __shared__ int wave_hits[kMaxWaves];
  const int i = threadIdx.x, lane = i & 63;
  const int wave = __builtin_amdgcn_readfirstlane(i >> 6);
  const int waves = (int)(blockDim.x >> 6);
  const int cursor = trace[0];          // every lane reads it before the barrier; lane 0 writes it after
  long id = -1;
  bool hit = false;
  if (i < Bn) {
    id = ids[i];
    // (an id outside the range never indexes the bitmap)
    if (id >= 0 && id < n_samples) hit = (tracked[id >> 5] >> (uint32_t)(id & 31)) & 1u;
  }
  const unsigned long long m = __ballot(hit);
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (lane == 0) wave_hits[wave] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < waves; ++w) {
    const int t = wave_hits[w];
    before += w < wave ? t : 0;
    total += t;
  }
  if (hit) {
    const long pos = (long)cursor + before + rank;
    if (pos >= 0 && pos < capacity) {       // a record past the capacity is dropped: counted, never written
      const float* row = tail + DAD_TAIL_HDR + i;
      i32x4 rec;
      rec[0] = epoch;
      rec[1] = (int32_t)id;
      rec[2] = ((int32_t)row[Bn] & 0xff) | (row[2 * (long)Bn] != 0.f ? DAD_TRACE_MASKED_IN : 0);
      rec[3] = __float_as_int(row[0]);
      *reinterpret_cast<i32x4*>(trace + DAD_TRACE_HDR_WORDS + pos * DAD_TRACE_REC_WORDS) = rec;
    }
  }
  if (i == 0) {
    const long offered = (long)cursor + total;     // saturates: the count never wraps to a small value
    trace[0] = offered > 0x7fffffffL ? 0x7fffffff : (int32_t)offered;
  }
}

extern "C" size_t dad_trace_bytes(int64_t capacity) {
  if (capacity < 0) capacity = 0;
  return (size_t)(DAD_TRACE_HDR_WORDS + capacity * DAD_TRACE_REC_WORDS) * sizeof(int32_t);
}

extern "C" int dad_trace_append(const float* tail, int Bn, const int64_t* ids, const uint32_t* tracked,
                                int64_t n_samples, int epoch, int32_t* trace, int64_t capacity, void* stream) {
  if (!tail || !ids || !tracked || !trace) return DAD_E_ARG;
  if (((uintptr_t)trace & 15u) != 0) return DAD_E_ARG;      // (the records are 16-byte stores)
  if (Bn < 1 || Bn > DAD_MAX_BATCH || n_samples < 1 || n_samples > 0x7fffffffLL || capacity < 0 ||
      capacity > 0x7fffffffLL)
    return DAD_E_SHAPE;
  const unsigned threads = (unsigned)((Bn + 63) / 64) * 64u;
  hipLaunchKernelGGL(dad_trace_append_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, tail, Bn, ids, tracked,
                     (long)n_samples, epoch, trace, (long)capacity);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DAD_OK : (int)e;
}
