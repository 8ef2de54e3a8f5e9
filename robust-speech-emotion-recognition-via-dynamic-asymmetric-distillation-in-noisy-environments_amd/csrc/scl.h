// The supervised-contrastive term (scl.hip) as the rest of the library sees it: where its rows come from, where its
// results go, its grid and its workspace.  dad_scl (dad.h) and the train step (dad_abi.hip) enqueue the same four
// launches through scl_enqueue.
#ifndef DAD_SCL_H_
#define DAD_SCL_H_
#include "dad_common.h"

// The n = na + nb rows of one call.  Rows [0, na): emb_a, an int64 label and a member byte each (mem_a NULL: every
// row is flagged).  Rows [na, n): emb_b, with the class and the flag as floats, the way the step's tail buffer holds
// the teacher's pseudo-label and the DACP mask (class = (int)pred_b, flagged = mask_b != 0).  nb may be 0.
struct SclSrc {
  const float* emb_a; const int64_t* lab_a; const uint8_t* mem_a; int na;
  const float* emb_b; const float* pred_b; const float* mask_b; int nb;
};

// What a call writes; every pointer may be NULL.
//   out    DAD_SCL_SLOTS floats
//   loss   one float, the loss (the step: tail[DAD_T_SCL])
//   grad   [n][256] dL/de, overwritten (rows outside the member set: 0)
//   acc, eflag, w   the step's hand-off (wgrad_common.h fused_ge1_v): for every member row u,
//          acc[u][:] = (eflag[u] ? acc[u][:] : 0) + w dL/de_u and eflag[u] = 1; other rows are left alone
struct SclDst {
  float* out; float* loss; float* grad;
  float* acc; uint32_t* eflag; float w;
};

// The grid of the two pairwise passes, (rt row tiles, chunks) workgroups: each row tile's rt column tiles in `chunks`
// runs of `per` (pairwise.h pair_plan).  scl_plan_of: one workgroup per compute unit (92 KB of LDS each);
// scl_plan_chunks: the chunk count asked for, clamped.  Host only.
struct SclPlan {
  int rt, chunks, per;
};
SclPlan scl_plan_of(int64_t n, int cus);
SclPlan scl_plan_chunks(int64_t n, int chunks);
size_t scl_ws_bytes(int64_t n);
inline bool scl_tau_ok(float tau) { return tau > 0.0f && tau <= 3.402823466e38f; }   // (NaN fails both)
// the four launches.  The arguments are the caller's to check.
int scl_enqueue(const SclSrc& src, const SclDst& dst, float tau, const SclPlan& pl, void* ws, hipStream_t stream);

#endif  // DAD_SCL_H_
