// swarm_pop_hp.hip — population training with one swarm_adam_cfg row per member
// (swarm_pop_train_tick_hp, swarm_pop_reduce_advance_hp): a learning-rate, gamma, clip, Adam or
// target-sync sweep in the population's two launches.  gfx950 only.
//
// Reference: src/training/train_gcn_dqn.py:262-290 runs one learner per seed under one set of
// hyper-parameters (:85 Adam(lr=1e-3), :112-137 gamma, clip_grad_norm_(1), update_target_every);
// a sweep over them is that loop run again per setting.  Here it is one population.
//
// The kernels are the statements of swarm_pop_tick_body.h / swarm_pop_reduce_body.h with HP = true: block (x, m) reads row m of member_hp with
// uniform loads issued beside its descriptor's (both addresses are a kernel argument plus
// blockIdx.y) and puts the row's optimizer fields where the bodies read them (ActArgs::hp,
// TdArgs::gamma, TdFused::hp, ReduceArgs::hp).  batch, world_size and flags stay the shared hp's:
// batch fixes the grid, S, grad_scale and the slab count, which one launch has once.  The
// instantiations live here, not in swarm_pop.hip, so that translation unit's code objects stay
// what they were (as swarm_qbk.hip does for the TD kernels).
#include "swarm_popk.h"

namespace swarm {

template <int NSA, int NST, int GS, int SCEN, int SPEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GS == 8 ? 2 : 3, GS == 8 ? 2 : 3))) void pop_tick_hp_kernel(
    const swarm_pop_member* __restrict__ members, const swarm_adam_cfg* __restrict__ member_hp, int B, int N, ActArgs A,
    TdArgs T, TdFused X) {
  constexpr bool HP = true;
#include "swarm_pop_tick_body.h"
}

__global__ __launch_bounds__(kRedCols * kRedGroups) void pop_reduce_hp_kernel(
    const swarm_pop_member* __restrict__ members, const swarm_adam_cfg* __restrict__ member_hp, int n_slabs,
    int env_offset, ReduceArgs A0) {
  constexpr bool HP = true;
#include "swarm_pop_reduce_body.h"
}

}  // namespace swarm

using namespace swarm;

extern "C" {

int swarm_pop_train_tick_hp(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                            const swarm_pop_member* members, int32_t n_members, void* stream) {
  if (!member_hp) return SWARM_E_BADARG;   // as members == NULL (a device table: its rows cannot be checked here)
  if (int e = check_pop(cfg, hp, members, n_members)) return e;
  const int B = cfg->n_envs, N = cfg->n_agents;
  const PopTickLaunch L = make_pop_tick(cfg, hp, n_members);
  with_tick_instance(cfg, [&](auto ns, auto sc, auto sp) {
    constexpr int NSA = decltype(ns)::value;
    hipLaunchKernelGGL((pop_tick_hp_kernel<NSA, td_wave_slots(NSA), NSA, decltype(sc)::value, decltype(sp)::value>),
                       L.grid, dim3(256), 0, (hipStream_t)stream, members, member_hp, B, N, L.a, L.t, L.x);
  });
  return (int)hipGetLastError();
}

int swarm_pop_reduce_advance_hp(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                                const swarm_pop_member* members, int32_t n_members, void* stream) {
  if (!member_hp) return SWARM_E_BADARG;
  if (int e = check_pop(cfg, hp, members, n_members)) return e;
  const ReduceArgs a = make_pop_reduce(cfg, hp);
  hipLaunchKernelGGL(pop_reduce_hp_kernel, dim3(reduce_grid_x(a.advance), n_members), dim3(kRedCols * kRedGroups), 0,
                     (hipStream_t)stream, members, member_hp, a.n_slabs, cfg->env_offset, a);
  return (int)hipGetLastError();
}

}  // extern "C"
