// swarm_gat3_bwd.hip — the gat3_backward_kernel instantiations (swarm_gat3_bwd.h), their slab
// reduce, the two launches and the entry point swarm_gat3_q_backward.  gfx950 only.
//
// Reference: loss.backward() through model(batch), src/training/train_gcn_dqn.py:122-124, for the
// GCN class with its conv2 / conv3 layers (:54-55, :65-68).
#include "swarm_launch.h"
#include "swarm_gat3_bwd.h"

namespace swarm {

// the slabs lie in the caller's swarm_td_workspace_floats(cfg, n_envs) floats: per slot class no
// more slabs than TD blocks (td_blocks), each no longer than a TD slab
constexpr bool g3b_slabs_fit(int gs) {
  return g3b_waves(gs) >= kTdRows / td_slots(gs) && (size_t)kG3Cols <= slab_floats_per_block();
}
static_assert(g3b_slabs_fit(8) && g3b_slabs_fit(16) && g3b_slabs_fit(32), "gat3 backward slabs fit the TD workspace");
static_assert(kG3Cols == SWARM_GAT3_GRAD_FLOATS && G3_N_PARAMS == SWARM_GAT3_N_PARAMS, "header");

// gat3_backward_kernel<NS> (the graph is read at run time, as in every GAT3 kernel), then the slab sum
int gat3_bwd_launch(const G3bArgs& A, hipStream_t stream) {
  with_slots<8, 16, 32>(A.N, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    hipLaunchKernelGGL((gat3_backward_kernel<NS>), dim3(A.n_slabs), dim3(64 * g3b_waves(NS)), 0, stream, A);
  });
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(gat3_grad_reduce_kernel<0>, dim3(kG3RedBlocks), dim3(kG3RedCols * kG3RedGroups), 0, stream,
                     (const float*)A.slabs, A.n_slabs, A.grad);
  return (int)hipGetLastError();
}

}  // namespace swarm

using namespace swarm;

extern "C" {

int swarm_gat3_q_backward(const swarm_config* cfg, const float* params, const float* x, const uint8_t* mult,
                          const float* dq, float* workspace, float* grad, void* stream) {
  if (int e = check_config(cfg, kCfgGat3Backward)) return e;
  if (cfg->net != SWARM_NET_GAT3) return SWARM_E_UNSUPPORTED;   // the one-layer network: swarm_q_backward
  if (!params || !x || !dq || !workspace || !grad) return SWARM_E_BADARG;
  if (cfg->graph == SWARM_GRAPH_DENSE && !mult) return SWARM_E_BADARG;
  G3bArgs a = {};
  a.B = cfg->n_envs; a.N = cfg->n_agents; a.graph = cfg->graph; a.k = cfg->knn_k; a.radius = cfg->radius;
  a.params = params; a.x = x; a.mult = mult; a.dq = dq; a.slabs = workspace; a.grad = grad;
  a.n_slabs = g3b_slabs(td_slots(a.N), a.B);
  return gat3_bwd_launch(a, (hipStream_t)stream);
}

}  // extern "C"
