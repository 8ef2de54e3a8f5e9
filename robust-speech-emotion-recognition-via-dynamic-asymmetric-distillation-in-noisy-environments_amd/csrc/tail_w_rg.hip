// dad_tail_ecda_w_rg: the wave-centric tail launch (tail_w.hip) of a ragged step (dad_config.ragged).  Its
// spare blocks pool the live slabs' partials only and prepare only the live rows of the next batch's noisy
// part, read from the feature store in its own type (f32, fp16 or bf16).  The same source compiled as a
// kernel and a unit of its own, as tail_w_s16.hip does.  (No stamps here: they belong to tail_w.hip.)
#undef DAD_PROBE_STAMPS
#define DAD_TAIL_W_RG 1
#include "tail_w.hip"
