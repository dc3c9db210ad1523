// swarm_pop_rollout.hip — population rollouts: P policies evaluated by ONE rollout launch
// (swarm_pop_rollout).  gfx950 only.
//
// Reference: src/simulation/simulator.py:59-93 (Simulator.run_simulation) runs one model on one
// environment; the evaluation grid runs it once per model seed on the same starts, and choosing a
// member of a trained population is one greedy rollout per member.  A rollout is a latency chain
// (one wave per environment, its state in registers for all n_ticks), and at the evaluation shape
// (1-8 environments per policy) a lone launch is one or two blocks.  Here blockIdx.y is the actor:
// block (x, m) does for actor m exactly what block x of swarm_rollout (swarm_act.hip) does, with
// the same body (act_body<NS, MODE_ROLLOUT, SCEN, SPEC, false, NET>) and the same kernel set
// (with_act_instance<MODE_ROLLOUT>, swarm_launch.h), so actor m computes a lone rollout's bits.
//
// An actor is a swarm_pop_actor descriptor in device memory (swarm_hip.h): the weights, the state,
// the outputs, the seed, tick0 and eps that swarm_rollout takes as arguments.  A block reads its
// descriptor first, with uniform (scalar) loads from &actors[blockIdx.y] (as pop_tick_kernel reads
// its member): one dependent round trip in front of the state and weight loads that the lone
// rollout issues from kernel arguments.  What all actors share (geometry, graph, conv, flags,
// n_ticks) stays in the kernel arguments.  Actors never exchange data.
//
// The instantiations live here, not in swarm_act.hip, so that translation unit's code objects stay
// what they were (as swarm_pop_hp.hip does for the population tick).
#include "swarm_popk.h"

namespace swarm {

// actor m's descriptor, read once with uniform loads; NULL stays NULL (load_member, swarm_popk.h)
__device__ inline swarm_pop_actor load_actor(const swarm_pop_actor* __restrict__ actors, unsigned int m) {
  swarm_pop_actor M = actors[m];
  M.params = as_global(M.params);
  M.state = as_global(M.state);
  M.out.q = as_global(M.out.q); M.out.actions = as_global(M.out.actions); M.out.reward = as_global(M.out.reward);
  M.out.obs = as_global(M.out.obs); M.out.avg_dist = as_global(M.out.avg_dist); M.out.hits = as_global(M.out.hits);
  M.out.mult = as_global(M.out.mult); M.out.traj_pos = as_global(M.out.traj_pos);
  M.out.traj_dist = as_global(M.out.traj_dist); M.out.traj_hits = as_global(M.out.traj_hits);
  return M;
}

// same block shape as act_kernel; A: the arguments of act_kernel with every per-actor field left empty
template <int NS, int SCEN, int SPEC, int NET>
__global__ __launch_bounds__(64 * kActWPB) void pop_rollout_kernel(const swarm_pop_actor* __restrict__ actors, int B,
                                                                  int N, ActArgs A) {
  __shared__ ActSmem<NS> S;
  const swarm_pop_actor M = load_actor(actors, blockIdx.y);
  ActArgs a = A;
  a.k0 = (uint32_t)(M.seed & 0xFFFFFFFFu); a.k1 = (uint32_t)(M.seed >> 32);
  a.params = M.params; a.state = M.state; a.out = M.out; a.tick0 = M.tick0; a.eps = M.eps;
  act_body<NS, MODE_ROLLOUT, SCEN, SPEC, false, NET>(S, blockIdx.x, gridDim.x, nullptr, M.state, nullptr, nullptr,
                                                     nullptr, nullptr, B, N, a);
}

}  // namespace swarm

using namespace swarm;

extern "C" {

int swarm_pop_rollout(const swarm_config* cfg, const swarm_pop_actor* actors, int32_t n_actors, int32_t n_ticks,
                      void* stream) {
  if (!cfg || !actors || n_actors < 1 || n_actors > 65535) return SWARM_E_BADARG;
  if (int e = check_config(cfg, kCfgActGraph)) return e;   // as swarm_rollout
  if (n_ticks < 0) return SWARM_E_BADARG;
  if (n_ticks == 0 || cfg->n_envs == 0) return 0;
  ActArgs a = make_act_args(cfg);
  a.k0 = 0; a.k1 = 0;   // the actor's
  a.n_ticks = n_ticks;
  const dim3 grid((a.B + kActWPB - 1) / kActWPB, n_actors), block(64 * kActWPB);
  with_act_instance<MODE_ROLLOUT>(a, [&](auto ns, auto sc, auto net, auto sp) {
    hipLaunchKernelGGL(
        (pop_rollout_kernel<decltype(ns)::value, decltype(sc)::value, decltype(sp)::value, decltype(net)::value>), grid,
        block, 0, (hipStream_t)stream, actors, a.B, a.N, a);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
