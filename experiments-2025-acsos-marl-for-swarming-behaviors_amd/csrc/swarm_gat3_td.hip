// swarm_gat3_td.hip — the gat3_td_kernel instantiations and gat3_adam_kernel (swarm_gat3_td.h),
// their launches and the entry points swarm_gat3_td_grad / swarm_gat3_adam_step.  gfx950 only.
//
// Reference: DQNTrainer.train_step_dqn, src/training/train_gcn_dqn.py:112-137, for the GCN class
// with its conv2 / conv3 layers (:54-55, :65-68).
#include "swarm_launch.h"
#include "swarm_gat3_td.h"

namespace swarm {

// the slabs lie in the caller's swarm_td_workspace_floats(cfg, hp->batch) floats: per slot class no
// more slabs than TD blocks of the same batch (td_blocks), each no longer than a TD slab
constexpr bool g3t_slabs_fit(int gs) {
  return g3b_waves(gs) >= kTdRows / td_slots(gs) && (size_t)kG3Cols <= slab_floats_per_block();
}
static_assert(g3t_slabs_fit(8) && g3t_slabs_fit(16) && g3t_slabs_fit(32), "gat3 TD slabs fit the TD workspace");
static_assert(kG3Cols == SWARM_GAT3_GRAD_FLOATS && G3_N_PARAMS == SWARM_GAT3_N_PARAMS, "header");

// no template: defined here, once, not in the header swarm_pop_gat3.hip includes too
__global__ __launch_bounds__(kG3AdamNT) void gat3_adam_kernel(G3AdamArgs A) {
  __shared__ float red[32];
  g3_adam_block(red, A);
}

// gat3_td_kernel<NS> (the graph is read at run time, as in every GAT3 kernel), then the slab sum
// with the loss column
int gat3_td_launch(const G3tArgs& A, hipStream_t stream) {
  with_slots<8, 16, 32>(A.N, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    hipLaunchKernelGGL((gat3_td_kernel<NS>), dim3(A.n_slabs), dim3(64 * g3b_waves(NS)), 0, stream, A);
  });
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(gat3_grad_reduce_kernel<1>, dim3(kG3RedBlocks), dim3(kG3RedCols * kG3RedGroups), 0, stream,
                     (const float*)A.slabs, A.n_slabs, A.grad);
  return (int)hipGetLastError();
}

int gat3_adam_launch(const G3AdamArgs& A, hipStream_t stream) {
  hipLaunchKernelGGL(gat3_adam_kernel, dim3(1), dim3(kG3AdamNT), 0, stream, A);
  return (int)hipGetLastError();
}

}  // namespace swarm

using namespace swarm;

extern "C" {

int swarm_gat3_td_grad(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* params, const float* target,
                       const swarm_replay* replay, const swarm_ctrl* ctrl, const int32_t* sample_in,
                       int32_t* sample_out, float* workspace, float* grad, void* stream) {
  if (int e = check_gat3_td(cfg, hp)) return e;
  if (!params || !target || !replay || !ctrl || !workspace || !grad) return SWARM_E_BADARG;
  if (!replay->s || !replay->s_next || !replay->r || !replay->a || replay->capacity < 1) return SWARM_E_BADARG;
  G3tArgs a = {};
  a.S = hp->batch; a.B = cfg->n_envs; a.N = cfg->n_agents; a.graph = cfg->graph; a.k = cfg->knn_k;
  a.env_offset = cfg->env_offset; a.k0 = seed_k0(cfg); a.k1 = seed_k1(cfg); a.radius = cfg->radius;
  a.gamma = hp->gamma;
  a.grad_scale = (float)(2.0 / ((double)hp->batch * (double)cfg->n_agents));   // MSELoss mean over the batch nodes
  a.params = params; a.target = target; a.replay = *replay; a.ctrl = ctrl;
  a.sample_in = sample_in; a.sample_out = sample_out; a.slabs = workspace; a.grad = grad;
  a.n_slabs = g3b_slabs(td_slots(a.N), a.S);
  return gat3_td_launch(a, (hipStream_t)stream);
}

int swarm_gat3_adam_step(const swarm_config* cfg, const swarm_adam_cfg* hp, float* params, float* target,
                         float* adam_m, float* adam_v, const float* grad, int32_t replay_capacity, swarm_ctrl* ctrl,
                         void* stream) {
  if (int e = check_gat3_td(cfg, hp)) return e;
  if (!params || !target || !adam_m || !adam_v || !grad || !ctrl || replay_capacity < 1) return SWARM_E_BADARG;
  G3AdamArgs a = {};
  a.hp = *hp; a.B = cfg->n_envs; a.N = cfg->n_agents; a.capacity = replay_capacity;
  a.params = params; a.target = target; a.m = adam_m; a.v = adam_v; a.grad = grad; a.ctrl = ctrl;
  return gat3_adam_launch(a, (hipStream_t)stream);
}

}  // extern "C"
