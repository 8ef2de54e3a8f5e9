// Host helpers shared by the translation units of the C ABI (dad_abi.hip, encoder_ops.hip).
#pragma once
#include "step_plan.h"

#define DAD_TRY(expr)                           \
  do {                                          \
    hipError_t e_ = (expr);                     \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

template <typename T>
inline T* ws_ptr(void* ws, size_t off) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off);
}

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

// compute units of the current device (cached per device)
int device_cus(int* out);
// standalone preparation of one set (dad_prep, prep_grid_of the current device)
// (ragged: dad_prep_rg, the preparation of a ragged step's set)
int launch_prep(const DadPrepArgs& p, hipStream_t stream, bool ragged = false);
