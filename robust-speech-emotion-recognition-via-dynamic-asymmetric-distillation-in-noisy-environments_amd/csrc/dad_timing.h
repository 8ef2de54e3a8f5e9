// Timing marks of the fused step (timing.hip): the step's enqueue code records these points.
#pragma once
#include "dad_common.h"
enum { TK_E0, TK_E1, TK_POOL, TK_TAIL, TK_WGRAD, TK_RED, TK_OPT0, TK_OPT1, TK_N };
void tk_begin();                          // a step starts (at its encoder call)
void tk_mark(int point, hipStream_t s);   // record point TK_* on s, if this step is timed
void tk_end();                            // the step is over (after its optimizer launch)
