// swarm_td.hip — learning side of the hot path: replay sample, TD loss, hand-written
// backward through GCN (PyG GATConv + MLP), deterministic gradient reduction,
// clip_grad_norm_ and Adam.  gfx950 only.
//
// Reference: DQNTrainer.train_step_dqn (src/training/train_gcn_dqn.py:112-137),
// GraphReplayBuffer.sample (:38-45), Adam(lr=1e-3) (:85), target sync (:131-133).
#include <stdlib.h>

#include "swarm_launch.h"
#include "swarm_peer.h"
#include "swarm_qbk.h"
#include "swarm_reduce.h"

namespace swarm {

// One TD block = 32 node slots (swarm_tdk.h).  The dependent chain's pointers (batch indices
// -> replay rows) and the geometry lead the parameter list: preloaded into SGPRs (kernarg
// preload), the index loads issue at wave start.
template <int NS, int GS, int SPEC>
__global__ __launch_bounds__(128 * (kTdRows / NS)) void td_kernel(const int32_t* sample_in, const float* rs,
                                                                  const float* rs_next, const float* rr,
                                                                  const uint8_t* ra, int S, int B, int N,
                                                                  int capacity, TdArgs A) {
  __shared__ TdSmem<NS> L;
  td_body<NS, GS, SPEC>(L, blockIdx.x, sample_in, rs, rs_next, rr, ra, S, B, N, capacity, A, TdFused{});
}

// ---------------------------------------------------------------- slab reduction (swarm_reduce.h;
// the block's statements: swarm_reduce_body.h, shared with swarm_pop.hip)
// slabs / ctrl / geometry preloaded into SGPRs (kernarg preload): the slab loads issue at wave start.
template <int PEER>
__global__ __launch_bounds__(kRedCols * kRedGroups) void grad_reduce_kernel(const float* slabs, swarm_ctrl* ctrl,
                                                                            int n_slabs, int advance, ReduceArgs A) {
#include "swarm_reduce_body.h"
}
// the one launch of grad_reduce_kernel: grid (reduce_grid_x, swarm_reduce.h), block, argument order
template <int PEER>
static int launch_reduce(const ReduceArgs& a, void* stream) {
  hipLaunchKernelGGL(grad_reduce_kernel<PEER>, dim3(reduce_grid_x(a.advance)), dim3(kRedCols * kRedGroups), 0,
                     (hipStream_t)stream, a.slabs, a.ctrl, a.n_slabs, a.advance, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- clip + Adam + target sync
// Unfused path (swarm_adam_step): apply now, then advance ctrl.  Flush path
// (swarm_adam_flush): apply a pending fused update in place, no advance.
struct AdamArgs {
  swarm_adam_cfg hp;
  int B, N, capacity, flush;
  float* params;
  float* target;
  float* m;
  float* v;
  const float* grad;
  swarm_ctrl* ctrl;
};

__global__ __launch_bounds__(kAdamNT) void adam_kernel(AdamArgs A) {
  __shared__ float red[64];
  const int tid = threadIdx.x;
  AdamRegs R;
  R.load(A.grad, A.params, A.m, A.v, tid);
  const float loss_sum = A.grad[N_PARAMS];
  swarm_ctrl* C = A.ctrl;
  const uint32_t cap = (uint32_t)A.capacity;
  const uint32_t filled = C->filled_slots;
  const uint32_t valid_slots = filled + 1 < cap ? filled + 1 : cap;
  const uint32_t tick = C->tick;
  const uint32_t step = C->adam_step + 1;
  const float step_size = C->adam_step_size, inv_bc2 = C->adam_inv_bc2;
  // ctrl words 24-25 (swarm_ctrl_init); a control block that skipped it holds 0 there: the
  // same value from the launch's hyper-parameters instead of freezing m and v
  const float one_m_b1 = C->one_m_beta1 != 0.0f ? C->one_m_beta1 : (float)(1.0 - adam_beta1(A.hp));
  const float one_m_b2 = C->one_m_beta2 != 0.0f ? C->one_m_beta2 : (float)(1.0 - adam_beta2(A.hp));
  const bool train = A.flush ? (C->trained != 0u && C->peer_hold == 0u)
                             : (valid_slots * (uint32_t)A.B >= (uint32_t)A.hp.batch);
  // target sync: unfused = after the TD step of tick `tick` ((tick+1) % every); flush = the
  // fused tick already advanced ctrl, so the pending update belongs to tick - 1
  const bool sync = ((A.flush ? tick : tick + 1) % (uint32_t)A.hp.update_target_every) == 0u;
  __syncthreads();   // every thread has read ctrl before thread 0 rewrites it
  float gn = 0.0f;
  if (train) {
    gn = adam_apply(R, A.hp, step_size, inv_bc2, one_m_b1, one_m_b2, tid, red);
    store4(A.params, R.w, R.wt, tid);
    store4(A.m, R.m, R.mt, tid);
    store4(A.v, R.v, R.vt, tid);
    if (sync) store4(A.target, R.w, R.wt, tid);
  }
  if (tid == 0) {
    if (train) {
      C->adam_step = step;
      C->grad_norm = gn;
      ctrl_set_double(C, CTRL_B1POW, ctrl_get_double(C, CTRL_B1POW) * adam_beta1(A.hp));
      ctrl_set_double(C, CTRL_B2POW, ctrl_get_double(C, CTRL_B2POW) * adam_beta2(A.hp));
      ctrl_store_next_scalars(C, A.hp);
      // (float)(1 - beta) of the next step from this launch's hp, as red_control rewrites it every
      // fused tick: after set_hp(betas=...) the old values act for this one step only, on every path
      C->one_m_beta1 = (float)(1.0 - adam_beta1(A.hp));
      C->one_m_beta2 = (float)(1.0 - adam_beta2(A.hp));
    }
    if (A.flush) {
      C->trained = 0u;
    } else {
      C->trained = 0u;   // applied now: nothing pending
      C->loss = train ? loss_sum / (float)((size_t)A.hp.batch * A.N) / (float)A.hp.world_size : 0.0f;
      if (!train) C->grad_norm = 0.0f;
      C->tick = tick + 1;
      C->write_slot = (C->write_slot + 1) % cap;
      C->filled_slots = valid_slots;
    }
  }
}

__global__ void ctrl_init_kernel(swarm_adam_cfg hp, float eps, swarm_ctrl* C) {
  uint32_t* w = reinterpret_cast<uint32_t*>(C);
  for (int i = 0; i < (int)(sizeof(swarm_ctrl) / 4); ++i) w[i] = 0u;
  C->eps = eps;
  C->sample_tick = 0xFFFFFFFFu;   // empty sampling-key cache
  C->one_m_beta1 = (float)(1.0 - adam_beta1(hp));   // torch: 1 - beta of Python floats
  C->one_m_beta2 = (float)(1.0 - adam_beta2(hp));
  ctrl_set_double(C, CTRL_B1POW, 1.0);
  ctrl_set_double(C, CTRL_B2POW, 1.0);
  ctrl_store_next_scalars(C, hp);
}

__global__ void ctrl_advance_kernel(swarm_ctrl* C, int capacity) {
  const uint32_t cap = (uint32_t)(capacity > 0 ? capacity : 1);
  C->tick = C->tick + 1;
  C->write_slot = (C->write_slot + 1) % cap;
  C->filled_slots = C->filled_slots + 1 < cap ? C->filled_slots + 1 : cap;
}

}  // namespace swarm

using namespace swarm;

namespace {
int check_td(const swarm_config* c, const swarm_adam_cfg* hp) { return check_config(c, kCfgTd, hp); }
}  // namespace

extern "C" {

int64_t swarm_td_workspace_floats(const swarm_config* cfg, int32_t batch) {
  if (!cfg || cfg->n_agents < 1 || cfg->n_agents > 32 || batch < 1) return SWARM_E_BADARG;
  return (int64_t)(td_blocks(cfg->n_agents, batch) * slab_floats_per_block());
}

int swarm_td_grad(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* params, const float* target,
                  const swarm_replay* replay, const swarm_ctrl* ctrl, const int32_t* sample_in, int32_t* sample_out,
                  float* slabs, void* stream) {
  if (int e = check_td(cfg, hp)) return e;
  if (!replay || !ctrl || !slabs || replay->capacity < 1) return SWARM_E_BADARG;
  const TdArgs a = make_td_args(cfg, hp, params, target, replay, ctrl, sample_in, sample_out, slabs);
  with_slots<8, 16, 32>(a.N, [&](auto gs) {
    constexpr int GS = decltype(gs)::value, NS = td_wave_slots(GS);
    with_spec<TdSpecs>(a.graph, a.conv, [&](auto sp) {
      hipLaunchKernelGGL((td_kernel<NS, GS, decltype(sp)::value>), dim3(a.n_slabs), dim3(128 * (kTdRows / NS)), 0,
                         (hipStream_t)stream, a.sample_in, a.replay.s, a.replay.s_next, a.replay.r, a.replay.a, a.S, a.B,
                         a.N, a.replay.capacity, a);
    });
  });
  return (int)hipGetLastError();
}

#if SWARM_STAMPS
int swarm_dbg_stamps_td(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_swarm_stamps), &p, sizeof(p)); }
#endif

int swarm_grad_reduce(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs, float* grad,
                      void* stream) {
  if (int e = check_td(cfg, hp)) return e;
  ReduceArgs a = {};
  a.n_slabs = td_blocks(cfg->n_agents, hp->batch); a.slabs = slabs; a.grad = grad;
  return launch_reduce<0>(a, stream);
}

// GCN.forward's backward for a caller's dL/dQ (swarm_qbk.h; kernels in swarm_qbk.hip), then the
// slab sum of swarm_grad_reduce
int swarm_q_backward(const swarm_config* cfg, const float* params, const float* x, const uint8_t* mult,
                     const float* dq, float* workspace, float* grad, void* stream) {
  if (int e = check_config(cfg, kCfgQBackward)) return e;
  if (!params || !x || !dq || !workspace || !grad) return SWARM_E_BADARG;
  if (cfg->graph == SWARM_GRAPH_DENSE && !mult) return SWARM_E_BADARG;
  QbArgs q = {};
  q.B = cfg->n_envs; q.N = cfg->n_agents; q.graph = cfg->graph; q.k = cfg->knn_k; q.conv = cfg->conv;
  q.radius = cfg->radius; q.params = params; q.x = x; q.mult = mult; q.dq = dq; q.slabs = workspace;
  q.n_slabs = td_blocks(q.N, q.B);
  if (int e = qbk_launch(q, (hipStream_t)stream)) return e;
  ReduceArgs a = {};
  a.n_slabs = q.n_slabs; a.slabs = workspace; a.grad = grad;
  return launch_reduce<0>(a, stream);
}

static int reduce_advance(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs, const swarm_learner* lr,
                          int32_t replay_capacity, swarm_ctrl* ctrl, const swarm_peer* peer, void* stream) {
  if (int e = check_td(cfg, hp)) return e;
  if (!lr || !ctrl || replay_capacity < 1) return SWARM_E_BADARG;
  ReduceArgs a = {};
  if (peer) a.peer = *peer;
  a.n_slabs = diag_reduce_slabs(td_blocks(cfg->n_agents, hp->batch)); a.slabs = slabs; a.grad = lr->grad;
  a.advance = 1; a.lr = *lr; a.ctrl = ctrl;
  a.capacity = replay_capacity; a.B = cfg->n_envs; a.N = cfg->n_agents; a.batch = hp->batch;
  a.hp = *hp;
  a.k0 = sample_salt_k0(seed_k0(cfg), cfg->env_offset); a.k1 = seed_k1(cfg);
  return peer ? launch_reduce<1>(a, stream) : launch_reduce<0>(a, stream);
}

int swarm_reduce_advance(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs, const swarm_learner* lr,
                         int32_t replay_capacity, swarm_ctrl* ctrl, void* stream) {
  return reduce_advance(cfg, hp, slabs, lr, replay_capacity, ctrl, nullptr, stream);
}

int swarm_reduce_advance_peer(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs,
                              const swarm_learner* lr, int32_t replay_capacity, swarm_ctrl* ctrl,
                              const swarm_peer* peer, void* stream) {
  if (int e = check_peer(peer)) return e;
  if (hp && hp->world_size != peer->world_size) return SWARM_E_BADARG;
  return reduce_advance(cfg, hp, slabs, lr, replay_capacity, ctrl, peer, stream);
}

static int launch_adam(const swarm_config* cfg, const swarm_adam_cfg* hp, float* params, float* target, float* m,
                       float* v, const float* grad, int32_t cap, swarm_ctrl* ctrl, int flush, void* stream) {
  AdamArgs a = {};
  a.hp = *hp; a.B = cfg->n_envs; a.N = cfg->n_agents; a.capacity = cap; a.flush = flush;
  a.params = params; a.target = target; a.m = m; a.v = v; a.grad = grad; a.ctrl = ctrl;
  hipLaunchKernelGGL(adam_kernel, dim3(1), dim3(kAdamNT), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

__global__ void sample_prepare_kernel(const swarm_ctrl* C, int capacity, int B, int batch, uint32_t k0, uint32_t k1,
                                      int32_t* out) {
  const uint32_t cap = (uint32_t)capacity;
  const uint32_t filled = C->filled_slots;
  const uint32_t vs = filled + 1 < cap ? filled + 1 : cap;
  const uint32_t ng = vs * (uint32_t)B;
  if (ng < (uint32_t)batch) return;
  const SampleKey sk = sample_key(ng, k0, k1, C->tick);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += gridDim.x * blockDim.x)
    out[i] = (int32_t)sample_index((uint32_t)i, sk);
}

int swarm_sample_prepare(const swarm_config* cfg, const swarm_adam_cfg* hp, int32_t replay_capacity,
                         const swarm_ctrl* ctrl, int32_t* samples, void* stream) {
  if (int e = check_td(cfg, hp)) return e;
  if (!ctrl || !samples || replay_capacity < 1) return SWARM_E_BADARG;
  hipLaunchKernelGGL(sample_prepare_kernel, dim3((hp->batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, ctrl,
                     replay_capacity, cfg->n_envs, hp->batch, sample_salt_k0(seed_k0(cfg), cfg->env_offset),
                     seed_k1(cfg), samples);
  return (int)hipGetLastError();
}

int swarm_adam_step(const swarm_config* cfg, const swarm_adam_cfg* hp, float* params, float* target, float* adam_m,
                    float* adam_v, const float* grad, int32_t replay_capacity, swarm_ctrl* ctrl, void* stream) {
  if (int e = check_td(cfg, hp)) return e;
  if (!params || !target || !adam_m || !adam_v || !grad || !ctrl || replay_capacity < 1) return SWARM_E_BADARG;
  return launch_adam(cfg, hp, params, target, adam_m, adam_v, grad, replay_capacity, ctrl, 0, stream);
}

int swarm_adam_flush(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_learner* lr, swarm_ctrl* ctrl,
                     void* stream) {
  if (int e = check_td(cfg, hp)) return e;
  if (!lr || !ctrl) return SWARM_E_BADARG;
  return launch_adam(cfg, hp, lr->w_cur, lr->target, lr->m_cur, lr->v_cur, lr->grad, 1, ctrl, 1, stream);
}

int swarm_ctrl_init(const swarm_adam_cfg* hp, float eps, swarm_ctrl* ctrl, void* stream) {
  if (!hp || !ctrl) return SWARM_E_BADARG;
  hipLaunchKernelGGL(ctrl_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, *hp, eps, ctrl);
  return (int)hipGetLastError();
}

int swarm_ctrl_advance(const swarm_config* cfg, const swarm_replay* replay, swarm_ctrl* ctrl, void* stream) {
  if (!cfg || !ctrl) return SWARM_E_BADARG;
  hipLaunchKernelGGL(ctrl_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctrl,
                     replay ? replay->capacity : 1);
  return (int)hipGetLastError();
}

}  // extern "C"
