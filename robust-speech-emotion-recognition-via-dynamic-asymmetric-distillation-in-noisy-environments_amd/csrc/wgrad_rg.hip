// dad_wgrad_direct[_f16][_cps]_rg: the direct weight gradient (wgrad.hip) of a ragged step
// (dad_config.ragged): the splits share the live slabs only, and the `_cps` forms skip the next batch's
// clean rows of dead slabs (wgrad_direct_body / wgd_tile, RG).  The same source compiled as kernels and a
// unit of their own, so that the dense kernels compile to what they did without the mode.  (The stamps
// build's buffer and readers belong to wgrad.hip: no stamps here.)
#undef DAD_PROBE_STAMPS
#define DAD_WGRAD_RG 1
#include "wgrad.hip"
