// swarm_popk.h — what the population kernels of swarm_pop.hip (one swarm_adam_cfg for all
// members, a kernel argument) and swarm_pop_hp.hip (one swarm_adam_cfg row per member, in device
// memory) share: the descriptor and row loads, the entry points' checks and kernel arguments.
// The kernels' statements themselves are swarm_pop_tick_body.h and swarm_pop_reduce_body.h.
#pragma once
#include "swarm_launch.h"
#include "swarm_reduce.h"

namespace swarm {

template <int NSA, int NST>
union PopSmem {
  ActSmem<NSA> a;
  TdSmem<NST> t;
};

// A pointer read from memory is a flat pointer to the compiler (only kernel arguments are known
// to be global), and a load through a flat pointer is never a scalar load, nor its result
// uniform.  Cast to the global address space and back, the loads behind it are global loads: of
// a uniform address, scalar ones, as in the lone tick, whose pointers are kernel arguments.  The
// empty asm keeps the two casts from being folded into nothing (as swarm_adam.h's tail loads
// do); it also pins the pointer, read with a uniform load, in SGPRs.  NULL stays NULL.
template <class T>
__device__ inline T* as_global(T* p) {
  typedef __attribute__((address_space(1))) T G;
  G* g = (G*)p;
  asm("" : "+s"(g));
  return (T*)g;
}
// member m's descriptor, read once with uniform loads; NULL stays NULL
__device__ inline swarm_pop_member load_member(const swarm_pop_member* __restrict__ members, unsigned int m) {
  swarm_pop_member M = members[m];
  M.state = as_global(M.state);
  M.replay.s = as_global(M.replay.s); M.replay.s_next = as_global(M.replay.s_next);
  M.replay.r = as_global(M.replay.r); M.replay.a = as_global(M.replay.a);
  M.lr.w_cur = as_global(M.lr.w_cur); M.lr.w_nxt = as_global(M.lr.w_nxt);
  M.lr.m_cur = as_global(M.lr.m_cur); M.lr.m_nxt = as_global(M.lr.m_nxt);
  M.lr.v_cur = as_global(M.lr.v_cur); M.lr.v_nxt = as_global(M.lr.v_nxt);
  M.lr.target = as_global(M.lr.target); M.lr.grad = as_global(M.lr.grad);
  M.ctrl = as_global(M.ctrl);
  M.out.q = as_global(M.out.q); M.out.actions = as_global(M.out.actions); M.out.reward = as_global(M.out.reward);
  M.out.obs = as_global(M.out.obs); M.out.avg_dist = as_global(M.out.avg_dist); M.out.hits = as_global(M.out.hits);
  M.out.mult = as_global(M.out.mult); M.out.traj_pos = as_global(M.out.traj_pos);
  M.out.traj_dist = as_global(M.out.traj_dist); M.out.traj_hits = as_global(M.out.traj_hits);
  M.slabs = as_global(M.slabs);
  M.workspace = as_global(static_cast<char*>(M.workspace));
  M.sample_out = as_global(M.sample_out);
  return M;
}
__device__ inline uint32_t member_k0(const swarm_pop_member& M) { return (uint32_t)(M.seed & 0xFFFFFFFFu); }
__device__ inline uint32_t member_k1(const swarm_pop_member& M) { return (uint32_t)(M.seed >> 32); }

// Member m's optimizer row.  Its address is a kernel argument plus blockIdx.y, so the loads are
// uniform (scalar) ones that need nothing of the descriptor: called in front of load_member, they
// are issued with the descriptor's loads and land with them.
__device__ inline swarm_adam_cfg load_member_hp(const swarm_adam_cfg* __restrict__ member_hp, unsigned int m) {
  return as_global(member_hp)[m];
}
// Called behind load_member (whose pointers the first wait is for anyway): the row's fields are in
// SGPRs from here on, so their loads are scalar loads that cannot sink into a later branch (where
// they would be a round trip of their own, and vector loads once a store precedes them).
__device__ inline void pin_member_hp(swarm_adam_cfg& r) {
  asm("" : "+s"(r.lr), "+s"(r.beta1), "+s"(r.beta2), "+s"(r.eps), "+s"(r.max_norm), "+s"(r.gamma),
           "+s"(r.update_target_every));
  asm("" : "+s"(r.lr_d), "+s"(r.beta1_d), "+s"(r.beta2_d));
}
// what a member's row decides: everything of the optimizer but batch, world_size and flags, which
// fix the grid, the slab count and the launch's own mode and stay the shared hp's
__device__ inline void take_member_hp(swarm_adam_cfg& hp, const swarm_adam_cfg& row) {
  hp.lr = row.lr; hp.beta1 = row.beta1; hp.beta2 = row.beta2; hp.eps = row.eps;
  hp.max_norm = row.max_norm; hp.gamma = row.gamma; hp.update_target_every = row.update_target_every;
  hp.lr_d = row.lr_d; hp.beta1_d = row.beta1_d; hp.beta2_d = row.beta2_d;
}

// what every population entry point checks before it launches, in this order
inline int check_pop(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members, int32_t n_members) {
  if (!cfg || !hp || !members || n_members < 1 || n_members > 65535) return SWARM_E_BADARG;
  if (hp->world_size != 1) return SWARM_E_BADARG;
  if (check_config(cfg, kCfgTick) != 0) return SWARM_E_UNSUPPORTED;   // as swarm_train_tick_supported
  if (hp->batch < 1 || hp->update_target_every < 1) return SWARM_E_BADARG;
  return 0;
}

// the kernel arguments both entry-point pairs launch with: every per-member field left empty
struct PopTickLaunch {
  ActArgs a;
  TdArgs t;
  TdFused x;
  dim3 grid;
};
inline PopTickLaunch make_pop_tick(const swarm_config* cfg, const swarm_adam_cfg* hp, int32_t n_members) {
  PopTickLaunch L;
  L.a = make_act_args(cfg);
  L.a.k0 = 0; L.a.k1 = 0;   // the member's
  L.a.learn = 1; L.a.hp = *hp;
  const swarm_replay no_replay = {};
  L.t = make_td_args(cfg, hp, nullptr, nullptr, &no_replay, nullptr, nullptr, nullptr, nullptr);
  L.t.k0 = 0; L.t.k1 = 0;
  L.x = {};
  L.x.hp = *hp;
  // per member the lone tick's grid; the kernel set of the fused tick
  L.grid = dim3(tick_grid_x(cfg->n_envs, L.t.n_slabs), n_members);
  return L;
}
inline ReduceArgs make_pop_reduce(const swarm_config* cfg, const swarm_adam_cfg* hp) {
  ReduceArgs a = {};
  a.n_slabs = diag_reduce_slabs(td_blocks(cfg->n_agents, hp->batch));
  a.advance = 1; a.B = cfg->n_envs; a.N = cfg->n_agents; a.batch = hp->batch; a.hp = *hp;
  return a;
}

}  // namespace swarm
