// Host helpers shared by the step's translation units of the C ABI (dad_abi.hip, encoder_ops.hip); DAD_TRY, DAD_RET,
// ws_ptr and device_cus, which the units outside the step use too, come from dad_common.h.
#pragma once
#include "step_plan.h"

struct Keys {
  uint32_t weak, strong, feat, tstart, drop1, drop2;
};

inline Keys keys_of(const dad_config* c) {
  Keys k;
  k.weak = dad_stream_key(c->seed, c->counter, DAD_RNG_WEAK);
  k.strong = dad_stream_key(c->seed, c->counter, DAD_RNG_STRONG);
  k.feat = dad_stream_key(c->seed, c->counter, DAD_RNG_FEAT);
  k.tstart = dad_stream_key(c->seed, c->counter, DAD_RNG_TSTART);
  k.drop1 = dad_stream_key(c->seed, c->counter, DAD_RNG_DROP1);
  k.drop2 = dad_stream_key(c->seed, c->counter, DAD_RNG_DROP2);
  return k;
}

// The KernelSig (step_plan.h) of a list of argument blocks; no other list can be launched.
template <typename... A> struct SigOf;
template <> struct SigOf<DadPrepArgs> { static constexpr KernelSig value = SIG_PREP; };
template <> struct SigOf<DadEncodeArgs> { static constexpr KernelSig value = SIG_ENCODE; };
template <> struct SigOf<DadPoolArgs> { static constexpr KernelSig value = SIG_POOL; };
template <> struct SigOf<DadTailArgs> { static constexpr KernelSig value = SIG_TAIL; };
template <> struct SigOf<DadTailArgs, DadEcdaArgs> { static constexpr KernelSig value = SIG_TAIL_ECDA; };
template <> struct SigOf<DadTailArgs, DadEcdaArgs, DadPrepArgs, DadPoolArgs> { static constexpr KernelSig value = SIG_TAIL_W; };
template <> struct SigOf<DadWgradArgs, DadReduceArgs> { static constexpr KernelSig value = SIG_WGRAD; };
template <> struct SigOf<DadWgradArgs, DadReduceArgs, DadPrepArgs> { static constexpr KernelSig value = SIG_WGRAD_CP; };
template <> struct SigOf<DadReduceArgs> { static constexpr KernelSig value = SIG_REDUCE; };

// The launch table: the entry point of every StepKernel, from the list in step_plan.h (which holds the
// block size).  A row whose KernelSig in the list is not that of its entry point's parameters does not
// compile; the pointer is kept without its type and gets it back in launch(), from the same KernelSig.
template <KernelSig S, typename... A>
constexpr void (*entry_of(void (*fn)(A...)))(A...) {
  static_assert(SigOf<A...>::value == S, "the list's KernelSig is not that of the entry point's argument blocks");
  return fn;
}
#define DAD_X_LAUNCH(id, fn, family, sig, threads) reinterpret_cast<void (*)()>(entry_of<sig>(fn)),
void (*const kLaunch[K_COUNT])() = {DAD_STEP_KERNELS(DAD_X_LAUNCH)};
#undef DAD_X_LAUNCH

// The only launch of a step kernel: k with the argument blocks of its KernelSig.  A kernel that takes
// other blocks is refused (DAD_E_ARG), not launched.
template <typename... A>
inline int launch(StepKernel k, int grid, hipStream_t stream, const A&... args) {
  if (kStepKernels[k].sig != SigOf<A...>::value) return DAD_E_ARG;
  hipLaunchKernelGGL(reinterpret_cast<void (*)(A...)>(kLaunch[k]), dim3(grid), dim3(kStepKernels[k].threads), 0, stream,
                     args...);
  DAD_TRY(hipGetLastError());
  return DAD_OK;
}

// standalone preparation of one set by preparation kernel k (prep_kernel; prep_grid_of the current device)
inline int launch_prep(StepKernel k, const DadPrepArgs& p, hipStream_t stream) {
  int cus = 0;
  const int rc = device_cus(&cus);
  if (rc) return rc;
  return launch(k, prep_grid_of(cus), stream, p);
}
