// swarm_reduce.h — the deterministic slab reduction and the ctrl advance of one tick: argument
// block, geometry and the control block's advance.  The statements of a reduce block are in
// swarm_reduce_body.h; grad_reduce_kernel (swarm_td.hip: swarm_grad_reduce,
// swarm_reduce_advance[_peer]) and the population's reduce (swarm_pop.hip: one learner per
// blockIdx.y) both include them, so their sums have the same bits.
#pragma once
#include "swarm_adam.h"
#include "swarm_peer.h"
#include "swarm_wpg.h"

namespace swarm {

// ---------------------------------------------------------------- slab reduction
// block = 256 threads covers 64 columns; thread (col, part) sums a contiguous quarter
// of the slabs, quarters combined in order: fixed order -> bitwise reproducible.
struct ReduceArgs {
  int n_slabs;
  const float* slabs;
  float* grad;
  int advance;            // fused tick: copy *_nxt -> *_cur and advance ctrl
  swarm_learner lr;
  swarm_ctrl* ctrl;
  int capacity, B, N, batch;
  swarm_adam_cfg hp;
  uint32_t k0, k1;        // replay-sampling key (seed ^ rank salt)
  swarm_peer peer;        // PEER = 1: the all-reduce over the ranks' exchange buffers (swarm_peer.h)
};

// 1024 threads = 16 columns x 64 slab groups (105 column blocks: the 1.7 MB of freshly
// written slabs is read by many CUs at once, 16 KB each); group g sums a contiguous run of
// slabs with every load issued before the ordered adds, then the 64 group sums of a column
// are added in a fixed two-level order (8 runs of 8, then the 8 run sums): bitwise
// reproducible run to run.  Advance mode adds one control block (the last): it prepares
// and stores the whole ctrl update (Adam scalars of the next step in double, the next
// tick's sampling key) in parallel with the column blocks, so no column block waits on it.
// Three more blocks copy w / m / v _nxt -> _cur (one array each), beside the column blocks.
#ifndef SWARM_RED_GROUPS
#define SWARM_RED_GROUPS 64   // test builds: 16 (256-thread blocks, so 8 ranks' peer reduces fit one GPU)
#endif
constexpr int kRedCols = 16;      // columns per reduce block
constexpr int kRedGroups = SWARM_RED_GROUPS;   // slab groups per column (consecutive slabs each)
constexpr int kRedRuns = kRedGroups / 8;
constexpr int kRedChunk = 8;      // slabs per load chunk of a group
constexpr int kRedColBlocks = (N_PARAMS + 1 + kRedCols - 1) / kRedCols;
constexpr int kRedCopyBlocks = 3;
// a reduce launch's grid: the column blocks; advance mode adds the control block and the copy blocks
constexpr int reduce_grid_x(int advance) { return kRedColBlocks + (advance ? 1 + kRedCopyBlocks : 0); }

// ---- the ctrl advance of one tick (the reduce launch's control block).  Every thread of the
//      block calls it; thread 0 advances the counters and the Adam scalars, thread 64 derives the
//      next tick's sampling key; both read ctrl before the barrier and write after it.
struct RedCtrl {
  int capacity, B, batch;
  swarm_adam_cfg hp;
  uint32_t k0, k1;   // replay-sampling key (seed ^ rank salt)
};

__device__ inline void red_control(swarm_ctrl* C, const RedCtrl& A) {
  const int t = threadIdx.x;
  uint32_t c_trained = 0, c_step = 0, c_tick = 0, c_slot = 0, c_filled = 0;
  double b1p = 1.0, b2p = 1.0;
  float next_step_size = 0.0f, next_inv_bc2 = 0.0f;
  SampleKey nk = {};
  uint32_t nk_n = 0, nk_tick = 0;
  const uint32_t cap = (uint32_t)A.capacity;
  if (t == 0) {
    // a held rank (peer_hold: an expired exchange wait) applied no step this tick
    c_trained = C->peer_hold ? 0u : C->trained;
    c_step = C->adam_step; c_tick = C->tick; c_slot = C->write_slot; c_filled = C->filled_slots;
    b1p = ctrl_get_double(C, CTRL_B1POW);
    b2p = ctrl_get_double(C, CTRL_B2POW);
    if (c_trained) {   // the step this tick's act kernel applied
      b1p = b1p * adam_beta1(A.hp);
      b2p = b2p * adam_beta2(A.hp);
      adam_next_scalars(A.hp, b1p, b2p, next_step_size, next_inv_bc2);
    }
  } else if (t == 64) {
    const uint32_t filled = C->filled_slots;
    const uint32_t f1 = filled + 1 < cap ? filled + 1 : cap;   // filled after this tick
    nk_n = (f1 + 1 < cap ? f1 + 1 : cap) * (uint32_t)A.B;       // graphs the next tick samples from
    nk_tick = C->tick + 1;
    nk = sample_key(nk_n, A.k0, A.k1, nk_tick);
  }
  __syncthreads();
  if (t == 0) {   // record the pending update, advance the tick
    const uint32_t valid_slots = c_filled + 1 < cap ? c_filled + 1 : cap;
    const uint32_t trained = valid_slots * (uint32_t)A.B >= (uint32_t)A.batch ? 1u : 0u;
    if (c_trained) {
      C->adam_step = c_step + 1;
      ctrl_set_double(C, CTRL_B1POW, b1p);
      ctrl_set_double(C, CTRL_B2POW, b2p);
      C->adam_step_size = next_step_size;
      C->adam_inv_bc2 = next_inv_bc2;
    }
    C->trained = trained;
    // (float)(1 - beta) of the Adam step, rewritten every tick from the launch's double
    // hyper-parameters: a control block that skipped swarm_ctrl_init (zero-filled) has its
    // first optimizer step pending only after this write, so no step runs with 0 here
    C->one_m_beta1 = (float)(1.0 - adam_beta1(A.hp));
    C->one_m_beta2 = (float)(1.0 - adam_beta2(A.hp));
    C->tick = c_tick + 1;
    C->write_slot = (c_slot + 1) % cap;
    C->filled_slots = valid_slots;
  } else if (t == 64) {
    C->sample_key[0] = nk.rk[0]; C->sample_key[1] = nk.rk[1]; C->sample_key[2] = nk.rk[2]; C->sample_key[3] = nk.rk[3];
    C->sample_bits = (uint32_t)nk.bits;
    C->sample_n = nk_n;
    C->sample_tick = nk_tick;
  }
}

static_assert(kRedGroups % 8 == 0 && kRedCols * kRedGroups <= 1024, "reduce geometry");
static_assert(kRedColBlocks <= kPeerSeqRegion, "peer seq region");
static_assert(kRedColBlocks == kGradSqCount && kRedCols == 16, "one norm partial per column block");

}  // namespace swarm
