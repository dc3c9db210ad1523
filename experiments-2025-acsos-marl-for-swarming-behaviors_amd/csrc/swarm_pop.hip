// swarm_pop.hip — population training: P independent learners ticked by ONE fused-tick launch
// and ONE reduce launch (swarm_pop_train_tick, swarm_pop_reduce_advance).  gfx950 only.
//
// Reference: the experiment of src/training/train_gcn_dqn.py:262-290 runs one learner (1 env,
// batch 32) per seed, seeds 0-9 one after another; at that shape a training tick is one acting
// block and eight TD blocks, about 1 % of the chip.  Here blockIdx.y is the population member:
// block (x, m) does for member m exactly what block x of swarm_train_tick (swarm_tick.hip) /
// swarm_reduce_advance (swarm_td.hip) does for a lone learner, with the same bodies
// (act_body, td_body, swarm_reduce_body.h), so member m computes a lone learner's bits.
//
// A member is a swarm_pop_member descriptor in device memory (swarm_hip.h): every pointer the
// lone tick takes as an argument, and the member's seed.  A block reads its descriptor first,
// with uniform (scalar) loads from &members[blockIdx.y]: one dependent round trip in front of the
// ctrl / weight / state loads that the lone tick issues from preloaded kernel arguments.  What
// all members share (geometry, graph, conv, flags, the Adam hyper-parameters) stays in the
// kernel arguments.
//
// The hand-off argument of the fused tick holds unchanged.  Blocks are dispatched in order of
// their linear index x + gridDim.x * m (x runs fastest).  A member's acting blocks are x in
// [0, n_act), its TD blocks x in [n_act, n_act + n_td): every acting block of member m has a
// lower linear index than every TD block of member m, and acting blocks never wait.  So when a
// TD block waits for a hand-off record, the acting block that publishes it has already been
// dispatched and runs to its end whatever else is resident: the wait ends even when
// P * (n_act + n_td) exceeds what the chip holds at once (the blocks of later members simply
// start as earlier ones drain).  Members never exchange data: a TD block only ever waits on its
// own member's records.  The wait stays the bounded one of the lone tick (kHoSpinLimit, counted
// in the member's workspace error word).
#include "swarm_popk.h"

namespace swarm {

// the kernels' statements are shared with swarm_pop_hp.hip as included files; same block shape
// and occupancy target as tick_kernel
template <int NSA, int NST, int GS, int SCEN, int SPEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GS == 8 ? 2 : 3, GS == 8 ? 2 : 3))) void pop_tick_kernel(
    const swarm_pop_member* __restrict__ members, int B, int N, ActArgs A, TdArgs T, TdFused X) {
  constexpr bool HP = false;
  constexpr const swarm_adam_cfg* member_hp = nullptr;
#include "swarm_pop_tick_body.h"
}

__global__ __launch_bounds__(kRedCols * kRedGroups) void pop_reduce_kernel(const swarm_pop_member* __restrict__ members,
                                                                           int n_slabs, int env_offset, ReduceArgs A0) {
  constexpr bool HP = false;
  constexpr const swarm_adam_cfg* member_hp = nullptr;
#include "swarm_pop_reduce_body.h"
}

}  // namespace swarm

using namespace swarm;

extern "C" {

int swarm_pop_train_tick(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members,
                         int32_t n_members, void* stream) {
  if (int e = check_pop(cfg, hp, members, n_members)) return e;
  const int B = cfg->n_envs, N = cfg->n_agents;
  const PopTickLaunch L = make_pop_tick(cfg, hp, n_members);
  with_tick_instance(cfg, [&](auto ns, auto sc, auto sp) {
    constexpr int NSA = decltype(ns)::value;
    hipLaunchKernelGGL((pop_tick_kernel<NSA, td_wave_slots(NSA), NSA, decltype(sc)::value, decltype(sp)::value>), L.grid,
                       dim3(256), 0, (hipStream_t)stream, members, B, N, L.a, L.t, L.x);
  });
  return (int)hipGetLastError();
}

int swarm_pop_reduce_advance(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members,
                             int32_t n_members, void* stream) {
  if (int e = check_pop(cfg, hp, members, n_members)) return e;
  const ReduceArgs a = make_pop_reduce(cfg, hp);
  hipLaunchKernelGGL(pop_reduce_kernel, dim3(reduce_grid_x(a.advance), n_members), dim3(kRedCols * kRedGroups), 0,
                     (hipStream_t)stream, members, a.n_slabs, cfg->env_offset, a);
  return (int)hipGetLastError();
}

}  // extern "C"
