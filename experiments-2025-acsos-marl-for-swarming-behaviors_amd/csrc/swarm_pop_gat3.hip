// swarm_pop_gat3.hip — populations of three-layer GAT learners: the unfused training tick of P
// SwarmGat3Engine-style learners in the four launches one of them costs (swarm_pop_gat3_act_step,
// swarm_pop_gat3_td_grad: two, swarm_pop_gat3_adam_step).  gfx950 only.
//
// Reference: src/training/train_gcn_dqn.py:262-290 runs the experiment once per seed (Flocking:
// ten seeds, one environment each, batch 32); the tick of one seed (:112-137, :161-172 with the
// GCN class's conv2 / conv3, :54-55, :65-68) is one acting block, 8 TD blocks, 26 reduce blocks
// and one 128-thread Adam block.  Here blockIdx.y is the member: block (x, m) does for member m
// what block x of swarm_act_step / swarm_gat3_td_grad / swarm_gat3_adam_step does, with the same
// statements (act_body, g3t_block, g3_reduce_block, g3_adam_block), block shapes, LDS layouts and
// slab layout, so member m computes a lone learner's bits.
//
// A member is a swarm_gat3_member descriptor in device memory (swarm_hip.h).  A block reads its
// descriptor first, with uniform (scalar) loads from &members[blockIdx.y] (as pop_rollout_kernel
// reads its actor): one dependent round trip in front of the loads the lone kernels issue from
// kernel arguments.  With HP the member's optimizer row comes from a device table the same way
// (load_member_hp, swarm_popk.h).  What all members share stays in the kernel arguments.
//
// The instantiations live here, not in swarm_act.hip / swarm_gat3_td.hip, so those translation
// units' code objects do not depend on these kernels (as swarm_pop_rollout.hip does for its own).
#include "swarm_popk.h"
#include "swarm_gat3_td.h"

namespace swarm {

// member m's descriptor, read once with uniform loads; NULL stays NULL (load_member, swarm_popk.h)
__device__ inline swarm_gat3_member load_gat3_member(const swarm_gat3_member* __restrict__ members, unsigned int m) {
  swarm_gat3_member M = members[m];
  M.state = as_global(M.state);
  M.replay.s = as_global(M.replay.s); M.replay.s_next = as_global(M.replay.s_next);
  M.replay.r = as_global(M.replay.r); M.replay.a = as_global(M.replay.a);
  M.params = as_global(M.params); M.target = as_global(M.target);
  M.adam_m = as_global(M.adam_m); M.adam_v = as_global(M.adam_v); M.grad = as_global(M.grad);
  M.ctrl = as_global(M.ctrl);
  M.out.q = as_global(M.out.q); M.out.actions = as_global(M.out.actions); M.out.reward = as_global(M.out.reward);
  M.out.obs = as_global(M.out.obs); M.out.avg_dist = as_global(M.out.avg_dist); M.out.hits = as_global(M.out.hits);
  M.out.mult = as_global(M.out.mult); M.out.traj_pos = as_global(M.out.traj_pos);
  M.out.traj_dist = as_global(M.out.traj_dist); M.out.traj_hits = as_global(M.out.traj_hits);
  M.slabs = as_global(M.slabs);
  M.sample_out = as_global(M.sample_out);
  return M;
}
__device__ inline uint32_t member_k0(const swarm_gat3_member& M) { return (uint32_t)(M.seed & 0xFFFFFFFFu); }
__device__ inline uint32_t member_k1(const swarm_gat3_member& M) { return (uint32_t)(M.seed >> 32); }

// same block shape as act_kernel; A: the arguments of act_kernel with every per-member field left empty
template <int NS, int SCEN>
__global__ __launch_bounds__(64 * kActWPB) void pop_gat3_act_kernel(const swarm_gat3_member* __restrict__ members,
                                                                   int B, int N, ActArgs A) {
  __shared__ ActSmem<NS> S;
  const swarm_gat3_member M = load_gat3_member(members, blockIdx.y);
  ActArgs a = A;
  a.k0 = member_k0(M); a.k1 = member_k1(M);
  a.params = M.params; a.state = M.state; a.replay = M.replay; a.ctrl = M.ctrl; a.out = M.out;
  act_body<NS, MODE_TICK, SCEN, SPEC_RUNTIME, false, SWARM_NET_GAT3>(S, blockIdx.x, gridDim.x, M.ctrl, M.state, nullptr,
                                                                    nullptr, nullptr, nullptr, B, N, a);
}

// gat3_td_kernel's block shape; A: its arguments with every per-member field left empty.  HP: gamma
// from member m's row
template <int NS, bool HP>
__global__ __launch_bounds__(64 * g3b_waves(NS)) void pop_gat3_td_kernel(const swarm_gat3_member* __restrict__ members,
                                                                        const swarm_adam_cfg* __restrict__ member_hp,
                                                                        G3tArgs A) {
  __shared__ G3tSmem<NS> L;
  // the row's loads first: they need nothing of the descriptor and are in flight beside its loads
  [[maybe_unused]] swarm_adam_cfg row;
  if constexpr (HP) row = load_member_hp(member_hp, blockIdx.y);
  const swarm_gat3_member M = load_gat3_member(members, blockIdx.y);
  if constexpr (HP) pin_member_hp(row);
  G3tArgs a = A;
  if constexpr (HP) a.gamma = row.gamma;
  a.k0 = member_k0(M); a.k1 = member_k1(M);
  a.params = M.params; a.target = M.target; a.replay = M.replay; a.ctrl = M.ctrl;
  a.sample_out = M.sample_out; a.slabs = M.slabs; a.grad = M.grad;
  g3t_block<NS>(L, blockIdx.x, a);
}

__global__ __launch_bounds__(kG3RedCols * kG3RedGroups) void pop_gat3_reduce_kernel(
    const swarm_gat3_member* __restrict__ members, int n_slabs) {
  __shared__ G3RedSmem L;
  const swarm_gat3_member M = load_gat3_member(members, blockIdx.y);
  g3_reduce_block<1>(L, blockIdx.x, G3RedArgs{M.slabs, n_slabs, M.grad});
}

// gat3_adam_kernel's block; A: its arguments with every per-member field left empty.  HP: the
// optimizer of member m's row (take_member_hp)
template <bool HP>
__global__ __launch_bounds__(kG3AdamNT) void pop_gat3_adam_kernel(const swarm_gat3_member* __restrict__ members,
                                                                 const swarm_adam_cfg* __restrict__ member_hp,
                                                                 G3AdamArgs A) {
  __shared__ float red[32];
  [[maybe_unused]] swarm_adam_cfg row;
  if constexpr (HP) row = load_member_hp(member_hp, blockIdx.y);
  const swarm_gat3_member M = load_gat3_member(members, blockIdx.y);
  if constexpr (HP) pin_member_hp(row);
  G3AdamArgs a = A;
  if constexpr (HP) take_member_hp(a.hp, row);
  a.capacity = M.replay.capacity;
  a.params = M.params; a.target = M.target; a.m = M.adam_m; a.v = M.adam_v; a.grad = M.grad; a.ctrl = M.ctrl;
  g3_adam_block(red, a);
}

// with_choice over a bool
template <class F>
void with_hp(bool hp, F&& f) {
  if (hp) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace swarm

using namespace swarm;

namespace {
// what the three entry points check first
int check_pop_gat3(const swarm_config* cfg, const void* members, int32_t n_members) {
  if (!cfg || !members || n_members < 1 || n_members > 65535) return SWARM_E_BADARG;
  return 0;
}
}  // namespace

extern "C" {

int swarm_pop_gat3_act_step(const swarm_config* cfg, const swarm_gat3_member* members, int32_t n_members,
                            void* stream) {
  if (int e = check_pop_gat3(cfg, members, n_members)) return e;
  if (int e = check_config(cfg, kCfgActGraph)) return e;   // as swarm_act_step
  if (cfg->net != SWARM_NET_GAT3) return SWARM_E_UNSUPPORTED;
  if (cfg->n_envs == 0) return 0;
  ActArgs a = make_act_args(cfg);
  a.k0 = 0; a.k1 = 0;   // the member's
  const dim3 grid((a.B + kActWPB - 1) / kActWPB, n_members), block(64 * kActWPB);
  with_slots<8, 16, 32>(a.N, [&](auto ns) {
    with_scenario(a.scenario, [&](auto sc) {
      hipLaunchKernelGGL((pop_gat3_act_kernel<decltype(ns)::value, decltype(sc)::value>), grid, block, 0,
                         (hipStream_t)stream, members, a.B, a.N, a);
    });
  });
  return (int)hipGetLastError();
}

int swarm_pop_gat3_td_grad(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                           const swarm_gat3_member* members, int32_t n_members, void* stream) {
  if (!hp) return SWARM_E_BADARG;
  if (int e = check_pop_gat3(cfg, members, n_members)) return e;
  if (int e = check_gat3_td(cfg, hp)) return e;
  G3tArgs a = {};
  a.S = hp->batch; a.B = cfg->n_envs; a.N = cfg->n_agents; a.graph = cfg->graph; a.k = cfg->knn_k;
  a.env_offset = cfg->env_offset; a.radius = cfg->radius;
  a.gamma = hp->gamma;
  a.grad_scale = (float)(2.0 / ((double)hp->batch * (double)cfg->n_agents));   // MSELoss mean over the batch nodes
  a.n_slabs = g3b_slabs(td_slots(a.N), a.S);
  hipStream_t st = (hipStream_t)stream;
  with_slots<8, 16, 32>(a.N, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    with_hp(member_hp != nullptr, [&](auto hpv) {
      hipLaunchKernelGGL((pop_gat3_td_kernel<NS, decltype(hpv)::value>), dim3(a.n_slabs, n_members),
                         dim3(64 * g3b_waves(NS)), 0, st, members, member_hp, a);
    });
  });
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(pop_gat3_reduce_kernel, dim3(kG3RedBlocks, n_members), dim3(kG3RedCols * kG3RedGroups), 0, st,
                     members, a.n_slabs);
  return (int)hipGetLastError();
}

int swarm_pop_gat3_adam_step(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                             const swarm_gat3_member* members, int32_t n_members, void* stream) {
  if (!hp) return SWARM_E_BADARG;
  if (int e = check_pop_gat3(cfg, members, n_members)) return e;
  if (int e = check_gat3_td(cfg, hp)) return e;
  G3AdamArgs a = {};
  a.hp = *hp; a.B = cfg->n_envs; a.N = cfg->n_agents;
  with_hp(member_hp != nullptr, [&](auto hpv) {
    hipLaunchKernelGGL(pop_gat3_adam_kernel<decltype(hpv)::value>, dim3(1, n_members), dim3(kG3AdamNT), 0,
                       (hipStream_t)stream, members, member_hp, a);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
