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

// A, T, X: the arguments of tick_kernel (swarm_tick.hip) with every per-member field left empty.
// Same block shape and occupancy target as tick_kernel.
template <int NSA, int NST, int GS, int SCEN, int SPEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GS == 8 ? 2 : 3, GS == 8 ? 2 : 3))) void pop_tick_kernel(
    const swarm_pop_member* __restrict__ members, int B, int N, ActArgs A, TdArgs T, TdFused X) {
  static_assert(64 * kActWPB == 256 && 128 * (kTdRows / NST) == 256, "one block shape for both halves");
  __shared__ PopSmem<NSA, NST> U;
  const swarm_pop_member M = load_member(members, blockIdx.y);
  const swarm_ctrl* const ctrl = M.ctrl;
  const swarm_learner lr = M.lr;
  const swarm_replay replay = M.replay;
  char* const ws = static_cast<char*>(M.workspace);
  // the member's fused-tick workspace: the error word's region, then the hand-off records (swarm_launch.h)
  unsigned long long* const rec = reinterpret_cast<unsigned long long*>(ws + kTickErrBytes);
  const int n_act = (B + kActWPB - 1) / kActWPB;
  if ((int)blockIdx.x < n_act) {
    ActArgs a = A;
    a.k0 = member_k0(M); a.k1 = member_k1(M);
    a.state = M.state; a.ctrl = ctrl; a.lr = lr; a.replay = replay; a.out = M.out;
    a.grad_norm_out = const_cast<float*>(&ctrl->grad_norm);
    a.ho_rec = rec;
    act_body<NSA, MODE_TICK, SCEN, SPEC, true, SWARM_NET_GCN>(U.a, blockIdx.x, n_act, ctrl, M.state, lr.grad, lr.w_cur,
                                                              lr.m_cur, lr.v_cur, B, N, a);
  } else {
    TdArgs t = T;
    t.k0 = member_k0(M); t.k1 = member_k1(M);
    t.params = lr.w_nxt; t.target = lr.target; t.replay = replay; t.ctrl = ctrl;
    t.sample_out = M.sample_out; t.slabs = M.slabs;
    TdFused x = X;
    x.lr = lr; x.ho_rec = rec; x.ho_err = reinterpret_cast<uint32_t*>(ws);
    td_body<NST, GS, SPEC, true>(U.t, (int)blockIdx.x - n_act, nullptr, replay.s, replay.s_next, replay.r, replay.a,
                                 t.S, B, N, replay.capacity, t, x, ctrl, lr.grad, lr.w_cur, lr.m_cur, lr.v_cur);
  }
}

// A0: the arguments of grad_reduce_kernel<0> in advance mode with every per-member field left
// empty; block (x, m) is block x of member m's reduce (the statements of swarm_reduce_body.h)
__global__ __launch_bounds__(kRedCols * kRedGroups) void pop_reduce_kernel(const swarm_pop_member* __restrict__ members,
                                                                           int n_slabs, int env_offset, ReduceArgs A0) {
  const swarm_pop_member M = load_member(members, blockIdx.y);
  constexpr int PEER = 0;
  const int advance = 1;
  ReduceArgs A = A0;
  A.slabs = M.slabs; A.grad = M.lr.grad; A.lr = M.lr; A.ctrl = M.ctrl; A.capacity = M.replay.capacity;
  A.k0 = sample_salt_k0(member_k0(M), env_offset); A.k1 = member_k1(M);
  const float* const slabs = A.slabs;
  swarm_ctrl* const ctrl = A.ctrl;
#include "swarm_reduce_body.h"
}

}  // namespace swarm

using namespace swarm;

namespace {
// what both entry points check before they launch, in this order
int check_pop(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members, int32_t n_members) {
  if (!cfg || !hp || !members || n_members < 1 || n_members > 65535) return SWARM_E_BADARG;
  if (hp->world_size != 1) return SWARM_E_BADARG;
  if (check_config(cfg, kCfgTick) != 0) return SWARM_E_UNSUPPORTED;   // as swarm_train_tick_supported
  if (hp->batch < 1 || hp->update_target_every < 1) return SWARM_E_BADARG;
  return 0;
}
}  // namespace

extern "C" {

int swarm_pop_train_tick(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members,
                         int32_t n_members, void* stream) {
  if (int e = check_pop(cfg, hp, members, n_members)) return e;
  const int B = cfg->n_envs, N = cfg->n_agents;
  ActArgs a = make_act_args(cfg);
  a.k0 = 0; a.k1 = 0;   // the member's
  a.learn = 1; a.hp = *hp;
  const swarm_replay no_replay = {};
  TdArgs t = make_td_args(cfg, hp, nullptr, nullptr, &no_replay, nullptr, nullptr, nullptr, nullptr);
  t.k0 = 0; t.k1 = 0;
  TdFused x = {};
  x.hp = *hp;
  // per member the lone tick's grid; the kernel set of the fused tick
  const dim3 grid(tick_grid_x(B, t.n_slabs), n_members), block(256);
  with_tick_instance(cfg, [&](auto ns, auto sc, auto sp) {
    constexpr int NSA = decltype(ns)::value;
    hipLaunchKernelGGL((pop_tick_kernel<NSA, td_wave_slots(NSA), NSA, decltype(sc)::value, decltype(sp)::value>), grid,
                       block, 0, (hipStream_t)stream, members, B, N, a, t, x);
  });
  return (int)hipGetLastError();
}

int swarm_pop_reduce_advance(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members,
                             int32_t n_members, void* stream) {
  if (int e = check_pop(cfg, hp, members, n_members)) return e;
  ReduceArgs a = {};
  a.n_slabs = diag_reduce_slabs(td_blocks(cfg->n_agents, hp->batch));
  a.advance = 1; a.B = cfg->n_envs; a.N = cfg->n_agents; a.batch = hp->batch; a.hp = *hp;
  hipLaunchKernelGGL(pop_reduce_kernel, dim3(reduce_grid_x(a.advance), n_members), dim3(kRedCols * kRedGroups), 0,
                     (hipStream_t)stream, members, a.n_slabs, cfg->env_offset, a);
  return (int)hipGetLastError();
}

}  // extern "C"
