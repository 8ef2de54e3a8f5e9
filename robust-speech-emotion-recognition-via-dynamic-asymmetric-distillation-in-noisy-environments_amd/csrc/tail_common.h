// What the tail launches share (device code, header only): the general path (tail_general.hip),
// the wave-centric path (tail_w.hip) and the helper-type kernels of utils_abi.hip.
//
//   * the block size and the ECDA row-group constants both ECDA forms index with
//   * fixed-order block reductions (block_sum_f, block_sum_d, block_sum4_d) and the general
//     tail's LDS layout (TailSmem, also dad_dacp_mask_kernel's)
//   * teacher softmax + certainty score (teacher_certainty, certainty_from_probs)
//   * the per-row arithmetic, ONE definition each, called by both paths, so their losses' rows,
//     thresholds and masks agree bit for bit by construction: the label-smoothed CE row (ce_row),
//     the masked KL row (kl_row) and the DACP threshold of one class (dacp_class_threshold).
//     What differs between the paths is how rows map to lanes and how partial sums are combined.
//   * dacp_thresholds: the general path's block-wide ranks around dacp_class_threshold
//
// Numerics: float32 with torch's op order where the result feeds a discrete decision
// (softmax -> certainty -> quantile -> EMA threshold -> mask); double accumulators for
// the batch sums.  The per-class set sizes are data dependent; everything is decided on
// device (no host sync), so the step is graph-capturable.
#pragma once
#include "dad_common.h"
#include "dad_kernels.h"

#define TAIL_THREADS DAD_TAIL_THREADS
#define ECDA_THREADS DAD_ECDA_THREADS
static_assert(ECDA_THREADS % DAD_H == 0 && ECDA_THREADS >= DAD_H, "ECDA column groups");
#define ECDA_NG (ECDA_THREADS / 64)         // row groups (one wave each) of the centroid pass
#define ECDA_PRE_U 8                        // rows per group held in registers from kernel entry

// v[k] of a 4-entry register array by a select chain (a run-time index would go through scratch)
__device__ __forceinline__ float sel4(const float (&v)[DAD_C], int k) {
  return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}
__device__ __forceinline__ int sel4i(const int (&v)[DAD_C], int k) {
  return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}
__device__ __forceinline__ double sel4d(const double (&v)[DAD_C], int k) {
  return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}

__device__ __forceinline__ float block_sum_f(float v, float* red) {
  v = dad_wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  float s = 0.0f;
  const int nw = blockDim.x >> 6;
  for (int k = 0; k < nw; ++k) s += red[k];
  return s;
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = dad_wave_sum_d(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  const int nw = blockDim.x >> 6;
  for (int k = 0; k < nw; ++k) s += red[k];
  return s;
}

// fixed-order block reduction of 4 doubles (one per class), result valid in all threads
__device__ __forceinline__ void block_sum4_d(double (&v)[4], double (*red)[4]) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = dad_wave_sum_d(v[c]);
  __syncthreads();
  if (l == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) red[w][c] = v[c];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double s = 0.0;
    for (int k = 0; k < TAIL_THREADS / 64; ++k) s += red[k][c];
    v[c] = s;
  }
}

struct TailSmem {
  double dred[16];
  double dred4[TAIL_THREADS / 64][4];
  float fred[16];
  float gz[2][DAD_MAX_BATCH][DAD_C];       // dL/dz clean, strong
  float sq[DAD_MAX_BATCH][DAD_C];          // teacher probs
  float ss[DAD_MAX_BATCH];                 // certainty scores
  int sp[DAD_MAX_BATCH];                   // pseudo labels
  float sm[DAD_MAX_BATCH];                 // mask
  float srt[DAD_C][DAD_MAX_BATCH];         // per-class sorted scores
  int ncls[DAD_C];
  float tau_new[DAD_C];
  float dstate[20];                        // DACP state: tau | Q | (sums) | (counts) | anchors
};

// DACPManager.calculate_certainty_scores (I/utils.py:400-428) of one probability row:
// pseudo-label = first argmax, score = max_prob * (1 - H / log2 C) with
// H = -sum q log2(q + 1e-8) (log2(NUM_CLASSES) = 2), or max_prob without the entropy term
__device__ __forceinline__ void certainty_from_probs(const float (&q)[4], bool entropy, float& s, int& pred) {
  float mx = -1.0f;
  pred = 0;
  for (int c = 0; c < 4; ++c)
    if (q[c] > mx) { mx = q[c]; pred = c; }
  s = mx;
  if (entropy) {
    float ent = 0.0f;
    for (int c = 0; c < 4; ++c) ent += q[c] * log2f(q[c] + 1e-8f);
    ent = -ent;
    s = mx * (1.0f - ent / 2.0f);
  }
}

// teacher probs (I/train.py:409-410), certainty score and pseudo-label (I/utils.py:400-428);
// the fixed-threshold branch (I/train.py:417-420) uses max_prob
__device__ __forceinline__ void teacher_certainty(const float (&z)[4], const dad_config& cfg, float (&q)[4],
                                                  float& s, int& pred) {
  float m = -INFINITY;
  for (int c = 0; c < 4; ++c) m = fmaxf(m, z[c]);
  float e[4], se = 0.0f;
  for (int c = 0; c < 4; ++c) { e[c] = expf(z[c] - m); se += e[c]; }
  for (int c = 0; c < 4; ++c) q[c] = e[c] / se;
  certainty_from_probs(q, cfg.use_dacp && cfg.use_entropy, s, pred);
}

// One row of the supervised CE with label smoothing eps over a batch of B (I/train.py:364,400):
// logits z, label y -> lse, g = dL/dz of the batch-mean loss, and the row's loss term in double.
__device__ __forceinline__ void ce_row(const float (&z)[4], int y, float eps, int B, float& lse, float (&g)[4],
                                       double& loss) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < 4; ++c) m = fmaxf(m, z[c]);
  float se = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) se += expf(z[c] - m);
  lse = m + logf(se);
  float lsum = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float ls = z[c] - lse;
    lsum += ls;
    const float pr = expf(ls);
    g[c] = (pr - (c == y ? 1.0f - eps : 0.0f) - eps * 0.25f) / (float)B;
  }
  const float zy = sel4(z, y);
  loss = -(1.0 - (double)eps) * (double)(zy - lse) - (double)eps * 0.25 * (double)lsum;
}

// One row of the masked consistency KL(q || p_student) (I/train.py:445-447): student logits z,
// teacher probs q, mask value mk (0 / 1), denom = mask sum + 1e-8 -> klb (unmasked row KL) and
// g = dL/dz (zero unless kl_on, I/train.py:444).
__device__ __forceinline__ void kl_row(const float (&z)[4], const float (&q)[4], float mk, bool kl_on, float w_kl,
                                       float denom, float& klb, float (&g)[4]) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < 4; ++c) m = fmaxf(m, z[c]);
  float se = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) se += expf(z[c] - m);
  const float lse = m + logf(se);
  klb = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float ls = z[c] - lse;
    const float t = q[c] * (logf(q[c]) - ls);
    klb += q[c] > 0.0f ? t : 0.0f;
    g[c] = kl_on ? w_kl * mk * (expf(ls) - q[c]) / denom : 0.0f;
  }
}

// The DACP threshold of class c (I/utils.py:449-507): n scores of the class sorted ascending in
// srt_c, quality scores Q, the class's threshold tau_c and calibrated anchor -> the sigmoid class
// weight wc, tau_hat (torch.quantile(linear); tau_c for an empty class), the floored value and
// the EMA-blended tau_new.  Branch-free: an empty class reads srt_c[0] and discards it.
__device__ __forceinline__ void dacp_class_threshold(const dad_config& cfg, int c, int n, const float* srt_c,
                                                     const float (&Q)[DAD_C], float tau_c, float anchor,
                                                     float& tau_new, float& wc, float& tau_hat, float& floored) {
  const float qmean = (((Q[0] + Q[1]) + Q[2]) + Q[3]) / 4.0f;
  wc = 1.0f / (1.0f + expf(-(cfg.dacp_k * (sel4(Q, c) - qmean))));
  // torch.quantile(linear): rank = q*(n-1) in f32, lerp(below, above, rank-floor)
  const float rank = cfg.dacp_gamma * (float)(n - 1);
  const int lo = (int)rank;
  const int hi = (int)ceilf(rank);
  const float wgt = rank - (float)lo;
  const float vlo = srt_c[lo < 0 ? 0 : lo], vhi = srt_c[hi < 0 ? 0 : hi];
  const float q = wgt < 0.5f ? vlo + wgt * (vhi - vlo) : vhi - (vhi - vlo) * (1.0f - wgt);
  tau_hat = n > 0 ? q : tau_c;
  const float adj = cfg.dacp_lambda * (wc - 0.5f);
  floored = fmaxf(tau_hat + adj, anchor);
  tau_new = cfg.dacp_alpha * tau_c + cfg.dacp_one_m_alpha * floored;
}

// DACPManager.calculate_mask thresholds (I/utils.py:449-507) by a whole block of the general
// path: per-class ranks of the scores (the class's scores sorted into srt[c]), then thread c
// takes class c's threshold (dacp_class_threshold).
// Entry: ncls[] zeroed and ss/sp visible (barrier done by the caller).  Exit: tau_new[] and
// wc[] valid in all threads.  tf/extras (nullable): the per-step outputs of the tail block.
// Shared by the tail block, the ECDA blocks of dad_tail_ecda and dad_dacp_mask_kernel.
template <int SRT = DAD_MAX_BATCH>
__device__ __forceinline__ void dacp_thresholds(const dad_config& cfg, int Bn, const float* ss, const int* sp,
                                                float (*srt)[SRT], int* ncls, const float* dstate,
                                                float* tau_new, float* wcs, float* tf, float* extras) {
  const int tid = threadIdx.x;
  // rank of each score inside its pseudo-label class (ties by index): 16 threads per
  // utterance, each counting a strided share of the others, combined by a 16-lane sum
  {
    const int bb = tid >> 4, part = tid & 15;
    for (int b0 = 0; b0 < Bn; b0 += TAIL_THREADS / 16) {
      const int b = b0 + bb;
      int cnt = 0, c = 0;
      float sv = 0.0f;
      if (b < Bn) {
        c = sp[b];
        sv = ss[b];
        int k = part;
        for (; k + 48 < Bn; k += 64) {   // four candidates per LDS round trip
          float o[4];
          int pc[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { o[u] = ss[k + 16 * u]; pc[u] = sp[k + 16 * u]; }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int kk = k + 16 * u;
            cnt += (pc[u] == c && (o[u] < sv || (o[u] == sv && kk < b))) ? 1 : 0;
          }
        }
        for (; k < Bn; k += 16) {
          const float o = ss[k];
          cnt += (sp[k] == c && (o < sv || (o == sv && k < b))) ? 1 : 0;
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 16);
      if (b < Bn && part == 0) {
        srt[c][cnt] = sv;
        atomicAdd(&ncls[c], 1);
      }
    }
  }
  __syncthreads();
  if (tid < DAD_C) {
    const int c = tid;
    const float Q[DAD_C] = {dstate[4], dstate[5], dstate[6], dstate[7]};
    float tn, wc, that, fl;
    dacp_class_threshold(cfg, c, ncls[c], srt[c], Q, dstate[c], dstate[16 + c], tn, wc, that, fl);
    tau_new[c] = tn;
    wcs[c] = wc;
    if (tf) {
      tf[DAD_T_W + c] = wc;
      tf[DAD_T_TAU_BEFORE + c] = dstate[c];
      tf[DAD_T_TAU_AFTER + c] = tn;
      tf[DAD_T_FLOORED + c] = fl;
      tf[DAD_T_TAU_HAT + c] = that;
      extras[0 + c] = fl;
    }
  }
  __syncthreads();
}
