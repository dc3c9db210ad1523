// swarm_diag.h — diagnostic timing knobs of the TD path, kept out of td_body (swarm_tdk.h) and the
// reduce's host code (swarm_td.hip).  Every hook is an identity in the product build (both knobs
// 0); an A/B build sets a knob with -D (tools/ab_build.py).
//   SWARM_DIAG_FEWSLABS = K > 0  only the first K TD blocks store their slab and the reduce reads
//                                K slabs: the timing bound of a slab cut (results are wrong)
//   SWARM_DIAG_FEWSLABS = -1     blocks on the pre path (holding a graph of this tick's slot) skip
//                                their slab stores; -2: the other blocks do.  The reduce reads all
//   SWARM_DIAG_PRE_ALL = 1       every TD block takes the pre path
#pragma once
#include <hip/hip_runtime.h>

#ifndef SWARM_DIAG_FEWSLABS
#define SWARM_DIAG_FEWSLABS 0
#endif
#ifndef SWARM_DIAG_PRE_ALL
#define SWARM_DIAG_PRE_ALL 0
#endif
// td_body's hooks (macros: a knob at 0 leaves no trace): state, does block vb store, the pre path
#if SWARM_DIAG_FEWSLABS > 0
#define TD_DIAG_SLAB_STATE
#define TD_DIAG_STORES_SLAB(vb) ((vb) < SWARM_DIAG_FEWSLABS)
#define TD_DIAG_SKIP_SET(pre)
#elif SWARM_DIAG_FEWSLABS < 0
#define TD_DIAG_SLAB_STATE bool diag_skip = false;   // set once the block knows its path
#define TD_DIAG_STORES_SLAB(vb) (!diag_skip)
#define TD_DIAG_SKIP_SET(pre) diag_skip = (SWARM_DIAG_FEWSLABS == -1) == (pre);
#else
#define TD_DIAG_SLAB_STATE
#define TD_DIAG_STORES_SLAB(vb) true
#define TD_DIAG_SKIP_SET(pre)
#endif
#if SWARM_DIAG_PRE_ALL
#define TD_DIAG_PRE(pre) \
  pre = true;               \
  TD_DIAG_SKIP_SET(pre)
#else
#define TD_DIAG_PRE(pre) TD_DIAG_SKIP_SET(pre)
#endif

namespace swarm {
// the reduce's hook: slabs it reads.  Only K > 0 cuts them; -1 / -2 keep every slab in the sum
inline int diag_reduce_slabs(int n_slabs) {
  return SWARM_DIAG_FEWSLABS > 0 && n_slabs > SWARM_DIAG_FEWSLABS ? SWARM_DIAG_FEWSLABS : n_slabs;
}
}  // namespace swarm
