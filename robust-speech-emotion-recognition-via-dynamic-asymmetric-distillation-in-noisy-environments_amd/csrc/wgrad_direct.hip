// dad_wgrad_direct[_f16][_cp|_cps|_cps_s16]: the dense entry points of the 16-bit direct weight gradient
// (wgrad_direct.h), and the stamps build's buffer.
#include "dad_probe.h"

// per-workgroup cycles of wave 0 in the stamps build (dad_probe.h): [prologue, loop, epilogue,
// -, sum over rounds of: compute+stage+load, barrier, -, -, rounds]
DAD_PROBE_BUFFER(wgd_stamps, 512 * 10)
#define WGD_CLK() DAD_PROBE_CLK()
#define WGD_ACC(k, v) \
  if (threadIdx.x == 0 && blockIdx.x < 512) DAD_PROBE_ADD(wgd_stamps, blockIdx.x * 10 + (k), (v))
#define WGD_ZERO()                                \
  for (int k = 0; DAD_PROBE_ON && k < 10; ++k)    \
    if (threadIdx.x == 0 && blockIdx.x < 512) DAD_PROBE_SET(wgd_stamps, blockIdx.x * 10 + k, 0)
#include "wgrad_direct.h"

WGD_KERNEL(dad_wgrad_direct, false, false)
WGD_KERNEL(dad_wgrad_direct_f16, true, false)
WGD_KERNEL_CP(dad_wgrad_direct_cp, false, WGD_CP_PADDED, false)
WGD_KERNEL_CP(dad_wgrad_direct_f16_cp, true, WGD_CP_PADDED, false)
WGD_KERNEL_CP(dad_wgrad_direct_cps, false, WGD_CP_STORE, false)
WGD_KERNEL_CP(dad_wgrad_direct_f16_cps, true, WGD_CP_STORE, false)
WGD_KERNEL_CP(dad_wgrad_direct_cps_s16, false, WGD_CP_STORE16, false)
WGD_KERNEL_CP(dad_wgrad_direct_f16_cps_s16, true, WGD_CP_STORE16, false)
