// dad_wgrad_direct[_f16][_cps]_rg: the direct weight gradient (wgrad_direct.h) of a ragged step
// (dad_config.ragged): the splits share the live slabs only, and the `_cps` forms skip the next batch's
// clean rows of dead slabs (wgrad_direct_body / wgd_tile, RG).  Kernels and a unit of their own, so that
// the dense kernels compile to what they did without the mode.  (The stamps build's buffer and readers
// belong to wgrad_direct.hip: no stamps here.)
#define WGD_CLK() 0ull
#define WGD_ACC(k, v) ((void)0)
#define WGD_ZERO() ((void)0)
#include "wgrad_direct.h"

WGD_KERNEL(dad_wgrad_direct_rg, false, true)
WGD_KERNEL(dad_wgrad_direct_f16_rg, true, true)
// (the next batch, ragged too, is a store batch; its rows' type is block-uniform)
WGD_KERNEL_CP(dad_wgrad_direct_cps_rg, false, WGD_CP_STORE, true)
WGD_KERNEL_CP(dad_wgrad_direct_f16_cps_rg, true, WGD_CP_STORE, true)
