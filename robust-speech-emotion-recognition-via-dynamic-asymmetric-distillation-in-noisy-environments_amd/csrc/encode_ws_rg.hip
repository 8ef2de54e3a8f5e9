// dad_encode_wp_rg / dad_encode_wp_f16_rg: the W-stationary encoder (encode_ws.hip) of a ragged step
// (dad_config.ragged), its jobs the live slabs only (encode_wp_body, RG).  The same source compiled as
// kernels and a unit of their own, so that the dense kernels compile to what they did without the mode.
// (The stamps build's buffer and readers belong to encode_ws.hip: no stamps here.)
#undef DAD_PROBE_STAMPS
#define DAD_ENC_WS_RG 1
#include "encode_ws.hip"
