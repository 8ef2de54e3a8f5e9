// dad_prep_rg: the standalone row preparation (prep.hip) of a ragged step (dad_config.ragged): the rows of
// dead slabs are skipped (dad_prep.h, RG); the store rows are read in their own type (f32, fp16 or bf16).
#include "dad_prep.h"

__global__ __launch_bounds__(DAD_PREP_THREADS) void dad_prep_rg(DadPrepArgs a) {
  DAD_GUARD_BLOCK(DAD_PREP_THREADS);
  if (!a.x16) return;
  constexpr int kWaves = DAD_PREP_THREADS / 64;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  dad_prep_dispatch<2, true, true>(a, (int)blockIdx.x * kWaves + w, (int)gridDim.x * kWaves, (int)threadIdx.x & 63);
}
