// The modular encoder operators of the C ABI (dad_encoder_forward / dad_encoder_backward) and the
// counter-RNG draws (dad_rng_draws).  Enqueue-only: no allocation, no synchronisation.
#include <string.h>

#include "dad_host.h"

// ------------------------------------------------------------------ counter-RNG draws
namespace {

// The throughput mode's random draws, by the device functions the step kernels call
// (dad_common.h): elements [first, first + n) of stream `which`.
__global__ __launch_bounds__(256) void dad_draws_kernel(int which, uint32_t key, uint64_t first, size_t n, float sd,
                                                        float p, float scale, int start_hi, float* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t e = first + i;
  float v = 0.0f;
  switch (which) {
    case DAD_DRAW_WEAK:
    case DAD_DRAW_STRONG: {
      float z0, z1;
      dad_aug_noise_pair(key, (uint32_t)(e >> 1), sd, z0, z1);
      v = (e & 1) ? z1 : z0;
      break;
    }
    case DAD_DRAW_FEAT_KEEP: v = dad_feat_keep(nullptr, key, (int)e, p); break;
    case DAD_DRAW_TSTART: v = (float)dad_tstart_at(key, (int)e, start_hi); break;
    default:   // DAD_DRAW_KEEP1 / KEEP2: element b * 256 + h
      v = keep_value(nullptr, key, (int)(e / DAD_H), (int)(e % DAD_H), p, scale);
      break;
  }
  out[i] = v;
}

}  // namespace

extern "C" {

int dad_rng_draws(const dad_config* cfg, int which, uint64_t first, size_t n, float* out, void* stream) {
  if (!cfg || (!out && n)) return DAD_E_ARG;
  const Keys k = keys_of(cfg);
  uint32_t key = 0;
  float sd = 0.0f, p = 0.0f;
  uint64_t limit = 0;
  const uint64_t noise = (uint64_t)cfg->Bn * (uint64_t)cfg->Tn * DAD_D;
  switch (which) {
    case DAD_DRAW_WEAK: key = k.weak; sd = cfg->weak_std; limit = noise; break;
    case DAD_DRAW_STRONG: key = k.strong; sd = cfg->strong_std; limit = noise; break;
    case DAD_DRAW_FEAT_KEEP: key = k.feat; p = cfg->feat_p; limit = DAD_D; break;
    case DAD_DRAW_TSTART: key = k.tstart; limit = (uint64_t)cfg->Bn; break;
    case DAD_DRAW_KEEP1: key = k.drop1; p = cfg->p_drop; limit = (uint64_t)cfg->B * DAD_H; break;
    case DAD_DRAW_KEEP2: key = k.drop2; p = cfg->p_drop; limit = (uint64_t)cfg->Bn * DAD_H; break;
    default: return DAD_E_ARG;
  }
  if (first + n > limit || limit > 0xffffffffull * 2) return DAD_E_SHAPE;
  if (n == 0) return DAD_OK;
  hipLaunchKernelGGL(dad_draws_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, which,
                     key, first, n, sd, p, cfg->drop_scale, cfg->start_hi, out);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

// ----------------------------------------------------------------- modular encoder ops
}  // extern "C"

// The modular encoder ops' workspace: the FP32 layout plus a prepared-row region (the 16-bit
// encoder's input: x converted by dad_prep).
static DadWs enc_layout(const DadGeom& G) {
  return dad_ws_layout(G, dad_auto_splits(G, DAD_PREC_FP32, 1), DAD_PREC_BF16);
}

extern "C" {
size_t dad_encoder_workspace_bytes(int B, int T) {
  if (B < 1 || T < 1) return 0;
  return enc_layout(dad_geom(B, T, 0, 0)).bytes;
}

}  // extern "C"

namespace {

__global__ __launch_bounds__(256) void dad_embed_kernel(const float* part_sum, const uint8_t* pad, int B, int T,
                                                        int nchunk, float* vlen, float* e_out) {
  (void)B;
  __shared__ float red[4];
  const int b = blockIdx.x, h = threadIdx.x;
  float l = 0.0f;
  for (int t = h; t < T; t += 256) l += pad[(size_t)b * T + t] == 0 ? 1.0f : 0.0f;
  l = dad_wave_sum(l);
  if ((h & 63) == 0) red[h >> 6] = l;
  __syncthreads();
  const float len = ((red[0] + red[1]) + red[2]) + red[3];
  float s = 0.0f;
  for (int c = 0; c < nchunk; ++c) s += part_sum[((size_t)b * nchunk + c) * DAD_H + h];
  e_out[(size_t)b * DAD_H + h] = s / fmaxf(len, 1.0f);
  if (h == 0 && vlen) vlen[b] = len;
}

// 16-bit copy of W1 in the W-stationary encoder's fragment order (dad_w1frag_index)
__global__ __launch_bounds__(256) void dad_w1h_kernel(const float* w, uint16_t* out, int f16) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)DAD_H * DAD_D)
    out[dad_w1frag_index((uint32_t)(i / DAD_D), (uint32_t)(i % DAD_D))] = dad_half_bits(w[i], f16 != 0);
}

int encoder_forward_impl(const float* x, const uint8_t* pad, int B, int T, const float* w1, const float* b1,
                         int precision, void* workspace, hipStream_t stream, const DadWs& L, float* vlen_out,
                         float* e_out) {
  uint16_t* w1h = ws_ptr<uint16_t>(workspace, L.w1h);
  const bool f16 = precision == DAD_PREC_FP16;
  if (dad_prec16(precision)) {
    hipLaunchKernelGGL(dad_w1h_kernel, dim3((DAD_H * DAD_D + 255) / 256), dim3(256), 0, stream, w1, w1h, f16 ? 1 : 0);
    DAD_TRY(hipGetLastError());
  }
  const DadGeom G = dad_geom(B, T, 0, 0);
  DadEncodeArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.g = G; ea.warmup = 1;
  ea.xc = x; ea.mc = pad; ea.w1_student = w1; ea.b1_student = b1; ea.w1h_student = w1h;
  ea.part_sum = ws_ptr<float>(workspace, L.part_sum);
  ea.part_cnt = ws_ptr<float>(workspace, L.part_cnt);
  ea.bits = ws_ptr<uint32_t>(workspace, L.bits);
  int grid = (B * G.ncc + 3) / 4;
  if (dad_prec16(precision)) {
    // the rows of x prepared (16-bit conversion: a clean-only set of a padded f32 batch), then the GEMM on them
    DadPrepArgs pp;
    memset(&pp, 0, sizeof(pp));
    pp.g = G; pp.warmup = 1; pp.clean = 1; pp.f16 = f16 ? 1 : 0; pp.xc = x;
    pp.x16 = ws_ptr<uint16_t>(workspace, L.xs16);
    DAD_RET(launch_prep(prep_kernel(false, false), pp, stream));
    ea.x16c = pp.x16;
    int cus = 0;
    DAD_RET(device_cus(&cus));
    DAD_RET(wp_split(G, 0, cus, ea.ws_nt, ea.ws_ns));
    grid = ea.ws_nt + ea.ws_ns;
  }
  DAD_RET(launch(encode_kernel(precision, false), grid, stream, ea));
  if (e_out) {
    hipLaunchKernelGGL(dad_embed_kernel, dim3(B), dim3(256), 0, stream, ea.part_sum, pad, B, T, G.ncc, vlen_out,
                       e_out);
    DAD_TRY(hipGetLastError());
  }
  return DAD_OK;
}

__global__ __launch_bounds__(256) void dad_embed_len_kernel(const uint8_t* pad, int B, int T, int nchunk,
                                                            const float* part_cnt, float* vlen, float* cnt_tot) {
  __shared__ float red[4];
  const int b = blockIdx.x, h = threadIdx.x;
  float l = 0.0f;
  for (int t = h; t < T; t += 256) l += pad[(size_t)b * T + t] == 0 ? 1.0f : 0.0f;
  l = dad_wave_sum(l);
  if ((h & 63) == 0) red[h >> 6] = l;
  __syncthreads();
  if (h == 0) vlen[b] = ((red[0] + red[1]) + red[2]) + red[3];
  float cnt = 0.0f;
  for (int c = 0; c < nchunk; ++c) cnt += part_cnt[((size_t)b * nchunk + c) * DAD_H + h];
  cnt_tot[(size_t)b * DAD_H + h] = cnt;
}

}  // namespace

extern "C" {

int dad_encoder_forward(const float* x, const uint8_t* pad, int B, int T, const float* w1, const float* b1,
                        float* e_out, int precision, void* workspace, void* stream) {
  if (!x || !pad || !w1 || !b1 || !e_out || !workspace) return DAD_E_ARG;
  if (B < 1 || B > DAD_MAX_BATCH || T < 1) return DAD_E_SHAPE;
  if (precision != DAD_PREC_FP32 && !dad_prec16(precision)) return DAD_E_ARG;
  const DadGeom G = dad_geom(B, T, 0, 0);
  const DadWs L = enc_layout(G);
  return encoder_forward_impl(x, pad, B, T, w1, b1, precision, workspace, (hipStream_t)stream, L,
                              ws_ptr<float>(workspace, L.vlen), e_out);
}

int dad_encoder_backward(const float* x, const uint8_t* pad, int B, int T, const float* w1, const float* b1,
                         const float* de, float* dw1, float* db1, void* workspace, void* stream_) {
  if (!x || !pad || !w1 || !b1 || !de || !dw1 || !db1 || !workspace) return DAD_E_ARG;
  if (B < 1 || B > DAD_MAX_BATCH || T < 1) return DAD_E_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const DadGeom G = dad_geom(B, T, 0, 0);
  const DadWs L = enc_layout(G);
  const int splits = L.splits;
  float* vlen = ws_ptr<float>(workspace, L.vlen);
  // recompute the ReLU'/valid bits and per-slab active counts (FP32 forward)
  int rc = encoder_forward_impl(x, pad, B, T, w1, b1, DAD_PREC_FP32, workspace, stream, L, nullptr, nullptr);
  if (rc) return rc;
  float* cnt_tot = ws_ptr<float>(workspace, L.cnt_tot);
  hipLaunchKernelGGL(dad_embed_len_kernel, dim3(B), dim3(256), 0, stream, pad, B, T, G.ncc,
                     ws_ptr<float>(workspace, L.part_cnt), vlen, cnt_tot);
  DAD_TRY(hipGetLastError());
  DadWgradArgs wa;
  memset(&wa, 0, sizeof(wa));
  wa.g = G; wa.warmup = 1; wa.splits = splits; wa.ntiles = 6 * splits;
  wa.xc = x; wa.bits = ws_ptr<uint32_t>(workspace, L.bits); wa.ge = de; wa.vlen = vlen;
  wa.wpart = ws_ptr<float>(workspace, L.wpart);
  DadReduceArgs none;
  memset(&none, 0, sizeof(none));
  DAD_RET(launch(K_WGRAD_F32, 6 * splits, stream, wa, none));
  float* gflat = ws_ptr<float>(workspace, L.gflat);
  DadReduceArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.g = G; ra.splits = splits; ra.warmup = 1; ra.want_norm = 0;
  ra.wpart = wa.wpart; ra.ge = de; ra.vlen = vlen; ra.cnt_tot = cnt_tot;
  ra.tailf = nullptr; ra.grad = gflat; ra.normpart = ws_ptr<float>(workspace, L.normpart);
  DAD_RET(launch(K_REDUCE, DAD_REDUCE_BLOCKS, stream, ra));
  DAD_TRY(hipMemcpyAsync(dw1, gflat + DAD_OFF_W1, sizeof(float) * DAD_H * DAD_D, hipMemcpyDeviceToDevice, stream));
  DAD_TRY(hipMemcpyAsync(db1, gflat + DAD_OFF_B1, sizeof(float) * DAD_H, hipMemcpyDeviceToDevice, stream));
  return DAD_OK;
}

}  // extern "C"
