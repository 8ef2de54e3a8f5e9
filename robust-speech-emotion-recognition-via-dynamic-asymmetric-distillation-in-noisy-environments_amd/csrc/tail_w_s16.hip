// dad_tail_ecda_w_s16: the wave-centric tail launch (tail_w.hip) whose spare blocks prepare the next
// batch's noisy rows from an fp16 / bf16 feature store, read in place (dad_prep.h, S16).  The same
// source compiled as a second kernel in a unit of its own: dad_tail_ecda_w then holds the f32
// preparation alone, and its tail and class blocks are compiled as before.  (The stamps build's
// buffers and readers belong to tail_w.hip: no stamps here.)
#undef DAD_PROBE_STAMPS
#define DAD_TAIL_W_S16 1
#include "tail_w.hip"
