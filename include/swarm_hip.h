/* swarm_hip.h — C ABI of libswarm_hip.so, the MI355X (gfx950) hot path of the
 * swarm-RL inner loop of davidedomini/experiments-2025-acsos-marl-for-swarming-behaviors.
 *
 * Conventions:
 *   - every buffer is caller-owned DEVICE memory, contiguous, fp32 / int32 / uint8;
 *   - `stream` is a hipStream_t passed as void* (0 = legacy default stream);
 *   - every entry point returns 0 on success, a positive hipError_t, or a
 *     negative SWARM_E_* code; nothing throws across the ABI;
 *   - no allocation, no host synchronisation inside any call: every call can be
 *     captured into a hipGraph (the one exception: the peer exchange's setup calls,
 *     swarm_peer_alloc / _free / _ipc_*, made once before any tick).
 *
 * Reference interfaces each entry point replaces are cited per function
 * (paths relative to the reference checkout; VMAS 1.4.0 / PyG 2.5.3 are the
 * reference's third-party dependencies, restated in SURVEY.md §8(a)).
 */
#ifndef SWARM_HIP_H
#define SWARM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWARM_ABI_VERSION 10

#define SWARM_E_BADARG (-1)    /* invalid shape / config */
#define SWARM_E_KNN_K (-2)     /* k > n_agents: torch.topk "selected index k out of range" */
#define SWARM_E_NOGPU (-3)
#define SWARM_E_UNSUPPORTED (-4) /* configuration has no fused-tick kernel (use the 3-launch tick) */

/* SWARM_FLOCKING: src/scenarios/flocking_scenario.py (the reference's third scenario class,
   train_gcn_dqn.py:244-245); needs n_agents >= 2 */
enum swarm_scenario { SWARM_GOTO = 0, SWARM_OBSTACLE_AVOIDANCE = 1, SWARM_FLOCKING = 2 };
enum swarm_graph { SWARM_GRAPH_COMPLETE = 0, SWARM_GRAPH_KNN = 1, SWARM_GRAPH_DENSE = 2, SWARM_GRAPH_RADIUS = 3 };
enum swarm_conv { SWARM_CONV_GAT = 0, SWARM_CONV_GCN = 1 };
/* Q-network: GCN = the reference's GCN class (one GATConv, hidden 32; params N_PARAMS = 1673;
   trainable).  GAT3 = the same class with its commented conv2/conv3 layers (train_gcn_dqn.py:54-55,
   65-68), hidden 8, 409 params: what data/models/experiment_Flocking-seed_*.pth hold.  GAT3 runs
   forward (swarm_q_forward, swarm_act_step, swarm_rollout), has the backward for a caller's
   dL/dQ (swarm_gat3_q_backward) and trains on the unfused device path through entry points of
   its own (swarm_act_step with a replay, swarm_gat3_td_grad, swarm_gat3_adam_step); the one-layer
   network's learner entry points (swarm_td_grad, swarm_adam_step, fused tick, populations) and
   swarm_q_backward return SWARM_E_UNSUPPORTED for it. */
enum swarm_net { SWARM_NET_GCN = 0, SWARM_NET_GAT3 = 1 };
#define SWARM_GAT3_N_PARAMS 409

/* Static description of a batch of vectorised environments (one rank's shard). */
typedef struct swarm_config {
  int32_t n_envs;       /* B: environments handled by this call                         */
  int32_t n_agents;     /* N: agents per environment, 1..32                             */
  int32_t scenario;     /* swarm_scenario                                               */
  int32_t graph;        /* swarm_graph: complete (train_gcn_dqn.py:101-108), kNN (simulator.py:15-24),
                           DENSE = caller-supplied multiplicity matrix [B][N][N] uint8, or
                           RADIUS = radius-neighbour graph (north_star):
                           edge u -> v for u != v with |p_u - p_v| <= radius, plus (0, 0)  */
  int32_t knn_k;        /* k of the kNN graph (reference code: 10, recorded data: 5)    */
  int32_t conv;         /* swarm_conv: GAT (the reference's GCN class) or GCNConv (a13) */
  int32_t env_offset;   /* global index of env 0 (rank sharding; keys the RNG)          */
  int32_t flags;        /* SWARM_F_* bits                                               */
  uint64_t seed;        /* Philox key                                                   */
  float radius;         /* neighbour radius of SWARM_GRAPH_RADIUS (> 0)                 */
  int32_t net;          /* swarm_net (GAT3 requires conv == SWARM_CONV_GAT)             */
} swarm_config;

#define SWARM_F_SHARED_RESET 1   /* one reset centre for all envs (go_to_position_scenario.py:88) */
#define SWARM_F_RANDOM_OA 2      /* ObstacleAvoidance random=True (obstacle_avoidance_scenario.py:100) */

/* Device-resident control block; kernels read and advance it so that a tick
 * sequence can be replayed from a captured hipGraph.  Layout is ABI. */
typedef struct swarm_ctrl {
  uint32_t tick;          /* completed ticks (the reference's `ticks` is tick + 1 during a tick) */
  uint32_t write_slot;    /* replay slot the next tick writes                               */
  uint32_t filled_slots;  /* valid replay slots, <= capacity                                */
  uint32_t adam_step;     /* optimizer steps taken                                          */
  float eps;              /* exploration epsilon for the next tick                          */
  float loss;             /* last TD loss (0 when the update was skipped)                   */
  float grad_norm;        /* last pre-clip global gradient norm                             */
  uint32_t trained;       /* 1 = an optimizer step is pending (fused tick: applied by the next
                             swarm_train_act_step or by swarm_adam_flush); 0 after swarm_adam_step */
  uint32_t episode;       /* episode counter (reset RNG key)                                */
  uint32_t pad0;
  uint32_t beta_pow[4];   /* beta1^adam_step, beta2^adam_step as two little-endian doubles
                             (words 10-13)                                                  */
  float adam_step_size;   /* Adam scalars of optimizer step adam_step + 1, kept current by the */
  float adam_inv_bc2;     /* library: lr / (1 - beta1^(s+1)) and 1 / sqrt(1 - beta2^(s+1))     */
  uint32_t sample_key[4]; /* cache: replay-sampling round keys of tick `sample_tick` over      */
  uint32_t sample_tick;   /* `sample_n` graphs, prepared by swarm_reduce_advance (words 16-22); */
  uint32_t sample_n;      /* recomputed from (tick, n) whenever the tags do not match          */
  uint32_t sample_bits;
  uint32_t peer_hold;     /* word 23, sticky: 1 once a peer-exchange wait of swarm_reduce_advance_peer
                             expired on this rank; every later optimizer step is then skipped (the
                             summed gradient is wrong), so a timeout never reaches the weights.
                             Cleared only by swarm_ctrl_init; PeerExchange.check() raises on it. */
  float one_m_beta1;      /* words 24-25: (float)(1 - beta1), (float)(1 - beta2) formed in double from   */
  float one_m_beta2;      /* swarm_adam_cfg's double betas by swarm_ctrl_init, as torch forms them, and
                             rewritten from the launch's swarm_adam_cfg by every
                             swarm_reduce_advance[_peer] and by every optimizer step that
                             swarm_adam_step / _flush apply; those two form them from their
                             swarm_adam_cfg when a word is 0 (a control block that skipped
                             swarm_ctrl_init), so no step freezes m and v.
                             After a change of swarm_adam_cfg between two optimizer steps, the first
                             step launched with the new values (the transition step, on every path
                             alike) takes from the control block what the launch before it wrote:
                             adam_step_size (the old lr over the old beta1's bias correction),
                             adam_inv_bc2 and one_m_beta1/2 (the old betas); it takes eps, max_norm
                             and v's decay factor beta2 from its own swarm_adam_cfg (the new ones).
                             So m moves by the old beta1 and v = new beta2 * v + (1 - old beta2) g^2
                             for that one step.  Every later step uses the new values throughout,
                             with bias corrections 1 - (the product of the beta each launch carried),
                             not 1 - beta^step.  gamma and update_target_every act at once.      */
  uint32_t pad1[6];
} swarm_ctrl;           /* 32 words */
/* A fresh control block comes from swarm_ctrl_init (all counters 0, beta powers 1). */

/* Replay ring (GraphReplayBuffer, train_gcn_dqn.py:25-48), SoA, per rank:
 * slot t holds the B transitions pushed at one tick. Graph id g = slot*B + env. */
typedef struct swarm_replay {
  float* s;          /* [cap][B][N][4]  state before the tick: pos.xy, vel.xy */
  float* s_next;     /* [cap][B][N][4]  state after the tick                 */
  float* r;          /* [cap][B][N]     per-agent reward                     */
  uint8_t* a;        /* [cap][B][N]     action                               */
  int32_t capacity;  /* slots                                                */
  int32_t pad;
} swarm_replay;

/* Per-tick outputs of the fused acting step; every pointer may be NULL. */
typedef struct swarm_act_out {
  float* q;          /* [B][N][9] Q-values                       */
  int32_t* actions;  /* [B][N] chosen actions                    */
  float* reward;     /* [B][N]                                   */
  float* obs;        /* [B][N][6] pos, vel, goal after the step  */
  float* avg_dist;   /* [B] scenario.average_distance_to_goal()  */
  float* hits;       /* [B] scenario.obstacles_hits()            */
  uint8_t* mult;     /* [B][N][N] edge multiplicity used         */
  float* traj_pos;   /* rollout only: [T][B][N][2] positions after every tick */
  float* traj_dist;  /* rollout only: [T][B] avg distance to goal per tick    */
  float* traj_hits;  /* rollout only: [T][B] obstacle hits per tick          */
} swarm_act_out;

/* Optimizer hyper-parameters (train_gcn_dqn.py:85,112-137). */
typedef struct swarm_adam_cfg {
  float lr, beta1, beta2, eps;   /* Adam(lr=1e-3), torch defaults                 */
  float max_norm;                /* clip_grad_norm_(…, 1)                          */
  float gamma;                   /* 0.99                                           */
  int32_t batch;                 /* sampled graphs per update (reference 32)       */
  int32_t update_target_every;   /* 200 at train_gcn_dqn.py:175                   */
  int32_t world_size;            /* ranks whose gradients are summed (grad /= W)   */
  int32_t flags;                 /* SWARM_ADAM_F_* (ABI 10; was padding)           */
  /* the same lr / betas in double, as torch.optim.Adam holds them (Python floats): 1 - beta
     (into the control block by swarm_ctrl_init) and the bias corrections are formed from these
     as torch forms them (ABI 9); 0 = use the float fields */
  double lr_d, beta1_d, beta2_d;
} swarm_adam_cfg;

/* swarm_adam_cfg.flags.  SWARM_ADAM_F_NORM_PARTIALS: the clip norm's group partials in lr->grad
 * (SWARM_GRAD_SQ_BASE, written by the slab reduce) belong to lr->grad as it is: the launch's
 * optimizer step then reads those 105 values instead of reducing the whole gradient behind a
 * block barrier (swarm_train_tick, swarm_train_act_step).  Set it when nothing changed lr->grad
 * after swarm_reduce_advance / _peer (one rank, or the fused peer exchange); clear it when an
 * all-reduce of the gradient (RCCL) or a caller wrote lr->grad in between.  Both ways give the
 * same bits: the partials are the same fixed-order sums the step forms otherwise. */
#define SWARM_ADAM_F_NORM_PARTIALS 1

/* Gradient buffers (swarm_learner.grad, the grad of swarm_grad_reduce / swarm_adam_step) hold
 * SWARM_GRAD_FLOATS floats: [0, N_PARAMS) the gradient, [N_PARAMS] the sum of squared TD errors,
 * then at SWARM_GRAD_SQ_BASE the clip norm's 105 group partials the slab reduce writes beside the
 * gradient (ABI 10): partial j = (d[4j] + d[4j+1]) + (d[4j+2] + d[4j+3]) over the float4 groups
 * d[i] = ((g0^2 + g1^2) + g2^2) + g3^2 of parameters 4i..4i+3 (each g scaled by 1/world_size when
 * world_size > 1; parameters >= N_PARAMS count 0); the squared norm is then
 * wave_sum(partial[l] + partial[l + 64]) over lanes l = 0..63 (swarm_adam.h). */
#define SWARM_GRAD_SQ_BASE 1680
#define SWARM_GRAD_SQ_COUNT 105
#define SWARM_GRAD_FLOATS 1792

/* Learner state for the fused training tick.  Weights/moments are ping-ponged so
 * that every block of swarm_train_act_step can read the previous tick's values
 * while block 0 persists the new ones: tick t reads *_cur, writes *_nxt;
 * swarm_reduce_advance copies *_nxt back to *_cur.  All buffers hold N_PARAMS
 * floats (grad: SWARM_GRAD_FLOATS, see above). */
typedef struct swarm_learner {
  float* w_cur;
  float* w_nxt;
  float* m_cur;
  float* m_nxt;
  float* v_cur;
  float* v_nxt;
  float* target;
  float* grad;
} swarm_learner;

int swarm_abi_version(void);
int swarm_n_params(void);                 /* 1673 */
const char* swarm_build_info(void);

/* Environment state: [B][N][4] floats (pos.xy, vel.xy) for every scenario.  SWARM_FLOCKING
 * keeps per-agent scenario state after it: [B][N] floats of previous_distance_to_agents
 * (flocking_scenario.py:110-122 at reset, :163-164 per reward call), which every entry point
 * that steps the env reads and writes.  swarm_state_floats gives the buffer size. */
int64_t swarm_state_floats(const swarm_config* cfg);

/* Reset: reset_world_at + generate_grid (go_to_position_scenario.py:52-106,
 * obstacle_avoidance_scenario.py:63-133, flocking_scenario.py:86-122) for all B envs. */
int swarm_env_reset(const swarm_config* cfg, float* state, uint32_t episode, void* stream);

/* Recompute the scenario state that follows [B][N][4] (Flocking; a no-op otherwise) from the
 * positions in `state`, after a caller wrote them: fresh != 0 as reset_world_at leaves it (the
 * reset loop measures agent i against the new positions of agents < i and the zeroed ones of
 * agents > i, flocking_scenario.py:93-122), fresh == 0 as a step's reward call leaves it. */
int swarm_env_sync_state(const swarm_config* cfg, float* state, int32_t fresh, void* stream);

/* VMAS Environment.step for discrete actions (call sites train_gcn_dqn.py:169,
 * simulator.py:68): decode, holonomic force, sphere collisions, drag/Euler,
 * scenario reward/observation/metrics.  actions [B][N] int32. */
int swarm_env_step(const swarm_config* cfg, float* state, const int32_t* actions,
                   const swarm_act_out* out, void* stream);

/* Graph build: DQNTrainer.create_graph_from_observations (train_gcn_dqn.py:94-110)
 * and simulator.create_graph_from_observations (simulator.py:9-26) as a dense
 * per-env edge multiplicity mult[b][u][v] = #edges u->v.  pos from x[:, :2]. */
int swarm_build_graph(const swarm_config* cfg, const float* x, uint8_t* mult, void* stream);

/* PyG edge_index [2][E] int64 of a Batch of n_graphs graphs with n_nodes nodes each
 * (Batch.from_data_list, train_gcn_dqn.py:45) -> dense multiplicity [G][N][N] uint8.
 * mult must be 4-byte aligned with room for roundup4(G*N*N) bytes; *err (device
 * int32) is set to 1 if an edge leaves its graph.  Multiplicities must stay < 256. */
int swarm_edges_to_mult(const int64_t* edge_index, int64_t n_edges, int32_t n_graphs,
                        int32_t n_nodes, uint8_t* mult, int32_t* err, void* stream);

/* GCN.forward (train_gcn_dqn.py:59-70) on B per-env graphs of N nodes.
 * x [B*N][7] node features; mult NULL unless cfg->graph == SWARM_GRAPH_DENSE. */
int swarm_q_forward(const swarm_config* cfg, const float* params, const float* x,
                    const uint8_t* mult, float* q, void* stream);

/* Backward of GCN.forward (train_gcn_dqn.py:59-70) for a caller-supplied dL/dQ: the torch
 * autograd of loss.backward() through model(batch) (train_gcn_dqn.py:122-124), parameters only.
 * x [B*N][7], mult as swarm_q_forward; dq [B*N][9] = dL/dQ.
 * grad[i] = sum over nodes n and actions a of dq[n][a] * dQ[n][a]/dtheta_i, flat PARAM_ORDER layout.
 * grad holds SWARM_GRAD_FLOATS floats: [N_PARAMS] is written 0, and the clip norm's partials at
 * SWARM_GRAD_SQ_BASE are written as by swarm_grad_reduce.
 * workspace: swarm_td_workspace_floats(cfg, cfg->n_envs) floats, need not be zeroed.
 * Two launches, no allocation, no host sync: capturable.
 * Bitwise reproducible run to run.  n_envs >= 1; SWARM_NET_GCN only (else SWARM_E_UNSUPPORTED:
 * the three-layer network's backward is swarm_gat3_q_backward). */
int swarm_q_backward(const swarm_config* cfg, const float* params, const float* x, const uint8_t* mult,
                     const float* dq, float* workspace, float* grad, void* stream);

/* The same for SWARM_NET_GAT3 (the Flocking checkpoints' three GATConvs, hidden 8): params [409],
 * x [B*N][7], mult as swarm_q_forward, dq [B*N][9].
 * grad holds SWARM_GAT3_GRAD_FLOATS floats: grad[i] = sum over nodes n and actions a of
 * dq[n][a] * dQ[n][a]/dtheta_i for i < 409 in the checkpoint's flat order, grad[409..415] = 0.
 * No norm partials (the caller clips).
 * workspace: swarm_td_workspace_floats(cfg, cfg->n_envs) floats, need not be zeroed.
 * Two launches, no allocation, no host sync: capturable.  Bitwise reproducible run to run.
 * Checks, in this order: the configuration as for swarm_q_forward but n_envs >= 1
 * (SWARM_E_BADARG / SWARM_E_KNN_K; GAT3 with GCNConv: SWARM_E_BADARG); net != SWARM_NET_GAT3:
 * SWARM_E_UNSUPPORTED (swarm_q_backward is that network's); a NULL params / x / dq / workspace /
 * grad: SWARM_E_BADARG; SWARM_GRAPH_DENSE with a NULL mult: SWARM_E_BADARG. */
#define SWARM_GAT3_GRAD_FLOATS 416   /* 409 gradients, then zeros */
int swarm_gat3_q_backward(const swarm_config* cfg, const float* params, const float* x, const uint8_t* mult,
                          const float* dq, float* workspace, float* grad, void* stream);

/* ---- The learner of SWARM_NET_GAT3 on the unfused device path (train_gcn_dqn.py:112-137 for the
 * three-layer network): per tick swarm_act_step (with the replay) -> swarm_gat3_td_grad ->
 * swarm_gat3_adam_step, four launches, what swarm_act_step -> swarm_td_grad -> swarm_grad_reduce ->
 * swarm_adam_step is for the one-layer network.  The fused tick, swarm_pop_member populations (PBT
 * among them) and world_size > 1 stay that network's; populations of these learners are ticked by
 * swarm_pop_gat3_act_step / _td_grad / _adam_step (below, after swarm_pop_rollout).
 *
 * swarm_gat3_td_grad: TD-loss gradient of a batch, the TD kernel + the slab sum, two launches.
 * Batch position i takes graph sample_in[i] (clamped to capacity * n_envs - 1) or, with sample_in
 * NULL, the graph swarm_td_grad would draw for it (the same keyed permutation of the
 * min(filled_slots + 1, capacity) * n_envs graphs in the ring, keyed by ctrl->tick); sample_out
 * [batch], if given, receives the ids.  One wave per graph: the target forward on s' (graph built
 * from the positions of s') gives y = r + gamma max_a Q_target, the online forward on s (graph from
 * s) gives td = Q[a] - y, and the backward of swarm_gat3_q_backward runs on dq = 2 td / (batch N)
 * at the taken action (MSELoss mean).  grad [SWARM_GAT3_GRAD_FLOATS]: [0, 409) the gradient in the
 * checkpoint's flat order, [409] the batch's sum of squared TD errors, [410..415] = 0.  While the
 * ring holds fewer than `batch` graphs the call writes grad = 0 (every slab column too) and
 * nothing else.  params / target hold 409 weights (SWARM_GAT3_GRAD_FLOATS floats where
 * swarm_gat3_adam_step takes them too).
 * workspace: swarm_td_workspace_floats(cfg, hp->batch) floats, need not be zeroed.
 * No atomics: bitwise reproducible.  No allocation, no host sync: capturable.
 *
 * swarm_gat3_adam_step: clip_grad_norm_(hp->max_norm) + Adam + target sync (when (tick + 1) %
 * update_target_every == 0) on the 409 parameters, then the control block advanced, in one launch:
 * swarm_adam_step's semantics field for field (the step runs iff min(filled_slots + 1,
 * replay_capacity) * n_envs >= batch; loss = grad[409] / (batch N) or 0; grad_norm or 0; trained
 * = 0; adam_step, the beta powers and the next step's scalars advanced when it ran; tick + 1,
 * write_slot advanced, filled_slots).  params, target, adam_m, adam_v hold SWARM_GAT3_GRAD_FLOATS
 * floats each; floats 409..415 are never used for a weight and are left as they are.
 *
 * Checks of both, in this order, all before any launch: the configuration and hp as swarm_td_grad /
 * swarm_adam_step check them (SWARM_E_BADARG / SWARM_E_KNN_K; GAT3 with GCNConv: SWARM_E_BADARG);
 * net != SWARM_NET_GAT3: SWARM_E_UNSUPPORTED; hp->world_size != 1: SWARM_E_UNSUPPORTED;
 * SWARM_GRAPH_DENSE: SWARM_E_BADARG (as for every TD entry point); a NULL pointer other than
 * sample_in / sample_out (the replay's four arrays among them), or a capacity < 1: SWARM_E_BADARG.
 * (tests/test_gat3_td_host.py, tests/test_gpu_gat3_td.py) */
int swarm_gat3_td_grad(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* params, const float* target,
                       const swarm_replay* replay, const swarm_ctrl* ctrl, const int32_t* sample_in,
                       int32_t* sample_out, float* workspace, float* grad, void* stream);
int swarm_gat3_adam_step(const swarm_config* cfg, const swarm_adam_cfg* hp, float* params, float* target,
                         float* adam_m, float* adam_v, const float* grad, int32_t replay_capacity,
                         swarm_ctrl* ctrl, void* stream);

/* Fused acting tick (train_gcn_dqn.py:161-172 / simulator.py:59-68):
 * graph -> GAT Q -> eps-greedy (ctrl->eps, Philox) -> env.step -> replay push
 * (replay may be NULL).  state updated in place. */
int swarm_act_step(const swarm_config* cfg, const float* params, float* state,
                   const swarm_replay* replay, const swarm_ctrl* ctrl,
                   const swarm_act_out* out, void* stream);

/* Fused training tick, acting half (train_gcn_dqn.py:161-172 + the optimizer step
 * of the previous tick's TD loss, :125-133): if ctrl->trained, apply
 * clip_grad_norm_ + Adam to (w_cur, grad) in every block (LDS image), block 0
 * persists w_nxt/m_nxt/v_nxt (+ target sync); then act with w_nxt.  If sample_out
 * != NULL it also draws this tick's TD batch indices [hp->batch] (exactly what
 * swarm_td_grad would draw in-kernel; pass them to it as sample_in).
 * Sequence per tick: swarm_train_act_step -> swarm_td_grad(params = w_nxt) ->
 * swarm_reduce_advance [-> all-reduce(grad)]. */
int swarm_train_act_step(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_learner* lr,
                         float* state, const swarm_replay* replay, const swarm_ctrl* ctrl,
                         const swarm_act_out* out, int32_t* sample_out, void* stream);

/* Fused training tick in ONE launch (train_gcn_dqn.py:153-178 without the optimizer's
 * launch): acting blocks (as swarm_train_act_step) and TD blocks (as swarm_td_grad with
 * in-kernel sampling) run side by side; both apply the pending optimizer step in registers.
 * TD graphs drawn from this tick's replay slot (the reference pushes before it samples,
 * :170-172) read the acting waves' write-through hand-off records in `workspace`
 * (swarm_train_tick_workspace_bytes; zero it whenever ctrl is (re)initialised).  Follow with
 * swarm_reduce_advance [-> all-reduce(grad)].  Bit-identical to the 3-launch sequence.
 * Complete, kNN or radius training graph, GAT or GCNConv, n_agents <= 16; else SWARM_E_UNSUPPORTED. */
int swarm_train_tick_supported(const swarm_config* cfg);
int64_t swarm_train_tick_workspace_bytes(const swarm_config* cfg);
int swarm_train_tick(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_learner* lr, float* state,
                     const swarm_replay* replay, const swarm_ctrl* ctrl, const swarm_act_out* out,
                     float* slabs, void* workspace, int32_t* sample_out, void* stream);

/* Host reference of the replay-batch permutation (GraphReplayBuffer.sample restated as a
 * keyed Feistel permutation; tests): index = batch position -> graph id, and its inverse. */
uint32_t swarm_host_sample_index(uint32_t i, uint32_t n, uint32_t k0, uint32_t k1, uint32_t tick);
uint32_t swarm_host_sample_position(uint32_t g, uint32_t n, uint32_t k0, uint32_t k1, uint32_t tick);

/* Slab sum -> lr->grad, copy *_nxt -> *_cur, record the pending update and
 * advance ctrl (tick, replay slot, the next step's Adam scalars). */
int swarm_reduce_advance(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs,
                         const swarm_learner* lr, int32_t replay_capacity, swarm_ctrl* ctrl, void* stream);

/* ---- Population training: P >= 1 independent learners ticked together (the reference runs its
 * experiment once per seed, train_gcn_dqn.py:262-290; a population runs the seeds side by side).
 * All members share one swarm_config except the seed (cfg->seed is ignored: each member's own
 * keys its Philox streams and its replay sampling) and one swarm_adam_cfg.  Each member owns
 * everything else, named by one descriptor: the arguments swarm_train_tick and
 * swarm_reduce_advance take for a lone learner.  The caller keeps an array of n_members
 * descriptors in DEVICE memory, written once.  Members never exchange data: member m computes
 * bit for bit what a lone learner with that seed computes with swarm_train_tick +
 * swarm_reduce_advance (tests/test_gpu_population.py). */
typedef struct swarm_pop_member {
  uint64_t seed;          /* the member's Philox key (what swarm_config.seed is to a lone learner) */
  float* state;           /* swarm_state_floats(cfg) floats                                        */
  swarm_replay replay;    /* the member's ring; replay.capacity is the member's own                */
  swarm_learner lr;
  swarm_ctrl* ctrl;
  swarm_act_out out;      /* any pointer may be NULL                                               */
  float* slabs;           /* swarm_td_workspace_floats(cfg, hp->batch) floats                      */
  void* workspace;        /* swarm_train_tick_workspace_bytes(cfg) bytes; zero it with ctrl        */
  int32_t* sample_out;    /* [hp->batch] this tick's TD batch indices, or NULL                     */
} swarm_pop_member;

/* The fused training tick of every member in ONE launch, grid (n_act + n_td, n_members): block
 * (x, m) does for member m what block x of swarm_train_tick does.  The configurations of
 * swarm_train_tick (else SWARM_E_UNSUPPORTED: n_agents > 16, GAT3, and every other configuration
 * swarm_train_tick_supported refuses, n_envs < 1 among them); hp->world_size must be 1 and
 * 1 <= n_members <= 65535 (else SWARM_E_BADARG, as for a NULL cfg, hp or members). */
int swarm_pop_train_tick(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members,
                         int32_t n_members, void* stream);
/* swarm_reduce_advance for every member in ONE launch, grid (105 + 1 + 3, n_members): member m's
 * slabs -> its lr.grad in the same fixed order (+ the clip norm's partials), *_nxt -> *_cur, and
 * its ctrl advanced with its own sampling key and replay.capacity.  Same checks as
 * swarm_pop_train_tick. */
int swarm_pop_reduce_advance(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_pop_member* members,
                             int32_t n_members, void* stream);

/* The same two launches with the optimizer's hyper-parameters PER MEMBER: a learning-rate, gamma,
 * clip, Adam or target-sync sweep run as one population (the reference fixes them for all seeds,
 * train_gcn_dqn.py:85,112-137,175, and runs once per seed, :262-290; a sweep is that loop again
 * per setting).  member_hp is an array of n_members swarm_adam_cfg in DEVICE memory; like
 * `members` it is written by the caller and read by the kernels on every launch, so a row
 * rewritten between two launches holds from the next launch on, the next replay of a captured
 * hipGraph included (a kernel-argument hp is frozen into the graph).
 *   per member, from row m : lr, beta1, beta2, eps, max_norm, gamma, update_target_every,
 *                            lr_d, beta1_d, beta2_d;
 *   shared, from *hp       : batch, world_size (= 1) and flags.  batch fixes the grid, the TD
 *                            batch size, the loss scale and the slab count, which a launch has
 *                            once.  These three fields of the rows are IGNORED.
 * Checks: those of swarm_pop_train_tick on cfg, hp, members and n_members, in the same order
 * (hp's own update_target_every >= 1 among them, though the rows' values are what the kernels
 * use); member_hp == NULL returns SWARM_E_BADARG, as members == NULL does.  The entry points
 * cannot look into device memory: every row must hold update_target_every >= 1 and finite values
 * (lr >= 0, eps >= 0, betas in [0, 1) as torch.optim.Adam asks, max_norm >= 0): that is the
 * caller's contract (SwarmPopulation enforces it).  Each member's control block comes from
 * swarm_ctrl_init with its own row, and its swarm_adam_flush takes its own row.  With all rows
 * equal to *hp both calls compute the bits of swarm_pop_train_tick / swarm_pop_reduce_advance
 * (tests/test_gpu_population_hp.py). */
int swarm_pop_train_tick_hp(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                            const swarm_pop_member* members, int32_t n_members, void* stream);
int swarm_pop_reduce_advance_hp(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                                const swarm_pop_member* members, int32_t n_members, void* stream);

/* ---- Peer all-reduce over xGMI (the one exchange of the data-parallel tick).
 * The reference has no distributed code; this replaces the RCCL all_reduce(grad) that would
 * follow swarm_reduce_advance (dist.py allreduce_grad_).  Every rank owns one exchange buffer
 * (swarm_peer_alloc: uncached device memory, so a peer's xGMI stores are seen by this GPU's
 * loads without a cache flush) and maps every other rank's buffer through HIP IPC.  A rank
 * publishes each gradient column as a tagged 8-byte granule {tag, value} with ONE system-scope
 * store into every rank's buffer (its own included) and polls its own buffer until all W tags
 * match: the data is its own flag.  The W values of a column are added in rank order, so every
 * rank computes bitwise the same sum.  Tags come from per-block launch counters (`seq`, device
 * words zeroed once at setup; every rank must issue the same sequence of peer calls) and the
 * buffer is double-buffered by their parity, so nothing is ever reset.  Waits are bounded in
 * time: one that expires adds 1 to *err (the sum is then wrong: check err and fail loudly); in
 * swarm_reduce_advance_peer it also sets ctrl->peer_hold, which stops every later optimizer step
 * of this rank before it can apply the wrong sum. */
#define SWARM_PEER_MAX 8
#define SWARM_PEER_HANDLE_BYTES 64   /* hipIpcMemHandle_t */
#define SWARM_PEER_SEQ_WORDS 256     /* launch counters per rank (device uint32, zeroed at setup) */
typedef struct swarm_peer {
  int32_t world_size;              /* W, 1..SWARM_PEER_MAX                                     */
  int32_t rank;                    /* this rank                                                */
  void* recv[SWARM_PEER_MAX];      /* rank q's exchange buffer as mapped in this process       */
  uint32_t* seq;                   /* SWARM_PEER_SEQ_WORDS launch counters of this rank        */
  int32_t* err;                    /* device int32: waits that hit the time bound              */
  uint32_t timeout_us;             /* bound of one wait (0 = 5 000 000 us: ranks start skewed) */
  int32_t pad;
} swarm_peer;

/* Setup (host-synchronous, not for the hot path): bytes of one exchange buffer; allocate one
 * (zeroed, uncached) / free it; export its IPC handle (SWARM_PEER_HANDLE_BYTES bytes); map a
 * peer's handle / unmap it. */
int64_t swarm_peer_buffer_bytes(void);
int swarm_peer_alloc(void** buf);
int swarm_peer_free(void* buf);
int swarm_peer_ipc_handle(void* buf, void* handle);
int swarm_peer_ipc_open(const void* handle, void** buf);
int swarm_peer_ipc_close(void* buf);

/* swarm_reduce_advance with the all-reduce fused in: each column block sums its slab columns,
 * exchanges them with the other ranks and writes lr->grad = the rank-ordered sum over ranks
 * (ctrl->loss stays this rank's own loss, as with swarm_reduce_advance + RCCL). */
int swarm_reduce_advance_peer(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs,
                              const swarm_learner* lr, int32_t replay_capacity, swarm_ctrl* ctrl,
                              const swarm_peer* peer, void* stream);

/* Standalone in-place SUM all-reduce of x[n] (n <= N_PARAMS + 1) over the ranks of `peer`
 * (rank-ordered, bitwise identical on every rank); the unfused API path's replacement of
 * all_reduce(grad), and the setup self-test. */
int swarm_peer_allreduce(const swarm_peer* peer, float* x, int32_t n, void* stream);

/* Draw the TD batch's replay indices [batch] for the tick ctrl describes
 * (GraphReplayBuffer.sample, train_gcn_dqn.py:40: keyed permutation, distinct ids). */
int swarm_sample_prepare(const swarm_config* cfg, const swarm_adam_cfg* hp, int32_t replay_capacity,
                         const swarm_ctrl* ctrl, int32_t* samples, void* stream);

/* Apply a pending update (ctrl->trained) to w_cur/m_cur/v_cur in place, e.g. after
 * the last fused tick.  No tick advance. */
int swarm_adam_flush(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_learner* lr,
                     swarm_ctrl* ctrl, void* stream);

/* Acting-only rollout of n_ticks ticks with frozen weights in ONE launch
 * (Simulator.run_simulation, simulator.py:59-93, greedy when eps = 0).
 * Tick t draws its coin and random actions with the key tick0 + t.  Of out (any pointer may be
 * null): reward [B][N] is each agent's sum over the ticks (fp32, in tick order); hits [B] is the
 * env's sum over the ticks; avg_dist [B] is the LAST tick's mean goal distance (Simulator's
 * "Distance (end)"), not a sum; obs [B][N][6] is the final observation (the state after the last
 * tick, then the goal); traj_pos / traj_dist / traj_hits hold every tick's positions, mean goal
 * distance and hits.  n_ticks = 0 returns 0 and writes nothing.
 * (tests/test_gpu_rollout_matrix.py) */
int swarm_rollout(const swarm_config* cfg, const float* params, float* state,
                  int32_t n_ticks, uint32_t tick0, float eps, const swarm_act_out* out, void* stream);

/* ---- Population rollouts: n_actors >= 1 policies evaluated in ONE launch (the reference's
 * evaluation grid runs Simulator.run_simulation, simulator.py:59-93, once per model seed on the
 * same environments; picking a population member is a greedy rollout per member).  All actors
 * share one swarm_config except the seed (cfg->seed is not used).  Each actor owns the rest, named
 * by one descriptor: what swarm_rollout takes for a lone policy.  The caller keeps an array of
 * n_actors descriptors in DEVICE memory; the kernel reads it on every launch, so a descriptor
 * rewritten between two launches (tick0, eps, another params pointer ...) holds from the next
 * launch on, the next replay of a captured hipGraph included.  Actors never exchange data and
 * must not share a state or output buffer. */
typedef struct swarm_pop_actor {
  uint64_t seed;        /* Philox key of this actor's coin / random actions (cfg->seed is not used) */
  const float* params;  /* swarm_n_params() floats (409 for SWARM_NET_GAT3)                         */
  float* state;         /* swarm_state_floats(cfg) floats; advanced n_ticks ticks, as swarm_rollout does */
  swarm_act_out out;    /* any pointer may be NULL; same meaning and layout as swarm_rollout's      */
  uint32_t tick0;       /* tick t is keyed tick0 + t                                                */
  float eps;
} swarm_pop_actor;

/* swarm_rollout for every actor in ONE launch, grid (ceil(n_envs / 4), n_actors): block (x, m)
 * does for actor m what block x of swarm_rollout does, with the same kernel set, so actor m
 * computes bit for bit what swarm_rollout computes with cfg->seed = actors[m].seed and the
 * actor's params, state, tick0, eps and out (tests/test_gpu_pop_rollout.py).
 * Checks, in this order: a NULL cfg or actors, or n_actors outside 1..65535: SWARM_E_BADARG; then
 * every configuration returns what swarm_rollout returns for it; n_ticks < 0: SWARM_E_BADARG;
 * n_ticks = 0 or n_envs = 0 returns 0 and writes nothing.  The descriptors are device memory the
 * entry point cannot look into: valid pointers are the caller's contract. */
int swarm_pop_rollout(const swarm_config* cfg, const swarm_pop_actor* actors, int32_t n_actors,
                      int32_t n_ticks, void* stream);

/* ---- Populations of SWARM_NET_GAT3 learners: n_members >= 1 independent learners of the
 * three-layer network ticked together (the reference's Flocking experiment: ten seeds, one
 * environment each, batch 32, one after another, train_gcn_dqn.py:262-290), in the four launches
 * per tick that one of them costs with swarm_act_step -> swarm_gat3_td_grad -> swarm_gat3_adam_step.
 * All members share one swarm_config except the seed (cfg->seed is not used: each member's own keys
 * its Philox streams and its replay sampling) and hp->batch.  Each member owns the rest, named by
 * one descriptor: what the three lone entry points take.  The caller keeps an array of n_members
 * descriptors in DEVICE memory; the kernels read it on every launch, so a descriptor rewritten
 * between two launches holds from the next launch on, the next replay of a captured hipGraph
 * included.  Members never exchange data and must not share a buffer: member m computes bit for
 * bit what a lone learner with cfg->seed = members[m].seed computes with the three lone entry
 * points (tests/test_gpu_gat3_population.py). */
typedef struct swarm_gat3_member {
  uint64_t seed;          /* the member's Philox key (what swarm_config.seed is to a lone learner) */
  float* state;           /* swarm_state_floats(cfg) floats                                        */
  swarm_replay replay;    /* the member's ring; replay.capacity is the member's own                */
  float* params;          /* SWARM_GAT3_GRAD_FLOATS floats each: 409 weights (swarm_gat3_adam_step) */
  float* target;
  float* adam_m;
  float* adam_v;
  float* grad;            /* as swarm_gat3_td_grad's grad                                          */
  swarm_ctrl* ctrl;
  swarm_act_out out;      /* any pointer may be NULL                                               */
  float* slabs;           /* swarm_td_workspace_floats(cfg, hp->batch) floats                      */
  int32_t* sample_out;    /* [hp->batch] this tick's TD batch indices, or NULL                     */
} swarm_gat3_member;

/* swarm_act_step for every member in ONE launch, grid (ceil(n_envs / 4), n_members): block (x, m)
 * does for member m what block x of swarm_act_step does with the member's seed, params, state,
 * replay (the push included; a NULL replay.s pushes nothing), ctrl and out.
 * Checks, in this order, all before any launch: a NULL cfg or members, or n_members outside
 * 1..65535: SWARM_E_BADARG; then every configuration returns what swarm_act_step returns for it
 * (SWARM_E_BADARG / SWARM_E_KNN_K; GAT3 with GCNConv: SWARM_E_BADARG); net != SWARM_NET_GAT3:
 * SWARM_E_UNSUPPORTED; n_envs = 0 returns 0 and launches nothing. */
int swarm_pop_gat3_act_step(const swarm_config* cfg, const swarm_gat3_member* members, int32_t n_members,
                            void* stream);
/* swarm_gat3_td_grad for every member in TWO launches: the TD kernel with grid (slabs of the batch,
 * n_members), then the slab sum with grid (26, n_members); block (x, m) does what block x of the
 * lone launch does with member m's params, target, replay, ctrl, slabs, grad and sample_out.  The
 * batch is always drawn in-kernel, member m's seed in the sampling key (there is no sample_in); the
 * skip rule (fewer than `batch` graphs in the ring: grad = 0) is each member's own, from its ctrl.
 * swarm_pop_gat3_adam_step: swarm_gat3_adam_step for every member in ONE launch, grid (1,
 * n_members), the ring capacity from members[m].replay.capacity.
 * member_hp: NULL (every member runs *hp), or an array of n_members swarm_adam_cfg in DEVICE memory,
 * read on every launch like `members`: member m then takes from row m what
 * swarm_pop_train_tick_hp's members take (lr, beta1, beta2, eps, max_norm, gamma,
 * update_target_every, lr_d, beta1_d, beta2_d; gamma acts in the TD launch, the rest in the
 * optimizer's), while batch, world_size and flags stay *hp's and the rows' are IGNORED.  Valid rows
 * (update_target_every >= 1, finite values) are the caller's contract, as valid descriptors are.
 * With all rows equal to *hp both ways compute the same bits.
 * Checks of both, in this order, all before any launch: a NULL cfg, hp or members, or n_members
 * outside 1..65535: SWARM_E_BADARG; then the configuration and hp return what swarm_gat3_td_grad
 * returns for them (SWARM_E_BADARG / SWARM_E_KNN_K; GAT3 with GCNConv: SWARM_E_BADARG; net !=
 * SWARM_NET_GAT3: SWARM_E_UNSUPPORTED; hp->world_size != 1: SWARM_E_UNSUPPORTED; SWARM_GRAPH_DENSE:
 * SWARM_E_BADARG).  The descriptors are device memory the entry points cannot look into: valid
 * pointers are the caller's contract.  No atomics, no allocation, no host sync: bitwise
 * reproducible, capturable.  (tests/test_gat3_population_host.py) */
int swarm_pop_gat3_td_grad(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                           const swarm_gat3_member* members, int32_t n_members, void* stream);
int swarm_pop_gat3_adam_step(const swarm_config* cfg, const swarm_adam_cfg* hp, const swarm_adam_cfg* member_hp,
                             const swarm_gat3_member* members, int32_t n_members, void* stream);

/* ---- Population-based training (Jaderberg et al. 2017): exploit and explore on the device.  The
 * reference trains every seed under fixed hyper-parameters and never moves a learner
 * (train_gcn_dqn.py:85,112-137,262-290); this works on the tables of swarm_pop_train_tick_hp.
 * The n_replace worst members (children) each take over the learner, the optimizer state and the
 * hyper-parameter row of one of the n_replace best (parents) and perturb lr and / or gamma.
 *
 * score [n_members] floats, higher is better; parent [n_members] int32 (output); member_hp and
 * members as swarm_pop_train_tick_hp takes them.  All four are DEVICE memory.
 *
 * Ranking: rank(m) = #{ j : s_j > s_m, or s_j == s_m and j < m }, a NaN score counting as -inf
 * (NaN members are worst; among equals the lower index ranks better).  Parents are ranks
 * 0 .. n_replace-1, children ranks n_members-n_replace .. n_members-1; n_replace <= n_members / 2
 * keeps the two sets disjoint, so nothing that is written is read by anyone else.
 * Draws: child m draws one block w = philox4x32(round, m, 5, 0, k0, k1) (stream id 5; k0 / k1 the
 * low / high word of seed).  parent[m] = the member of rank (w.x * n_replace) >> 32; the lr factor
 * is perturb_lo if (w.y >> 8) * 2^-24 < 0.5f, else perturb_hi; the gamma factor likewise from w.z.
 * Every other member gets parent[m] = m and is not written at all.
 * Copy, parent p -> child c, through the descriptors' pointers: the seven learner rows
 * (swarm_n_params() floats each), lr.grad (SWARM_GRAD_FLOATS floats: a pending step of the child
 * is then the parent's pending step) and the control words of the optimizer: adam_step, loss,
 * grad_norm, trained, beta_pow[4], adam_step_size, adam_inv_bc2, one_m_beta1, one_m_beta2.  The
 * child keeps everything else: tick, write_slot, filled_slots, eps, episode, the sampling-key
 * cache, peer_hold, its ring, env state, workspace, slabs and outputs.
 * Explore: row c of member_hp becomes row p, then
 *   SWARM_PBT_F_LR   : lr_d = min(max(lr_d_p * (double)f, lr_min), lr_max), with (double)lr_p in
 *                      place of lr_d_p where lr_d_p == 0; lr = (float)lr_d;
 *   SWARM_PBT_F_GAMMA: gamma = min(max(1.0f - (1.0f - gamma_p) * f, gamma_min), gamma_max), fp32.
 * That is "load the parent's optimizer state, then rewrite the child's row": the control block's
 * next-step scalars are the parent's, so the new lr acts one optimizer step later.
 *
 * Checks, in this order, before any launch: a NULL pbt, score, member_hp, members or parent:
 * SWARM_E_BADARG; n_members < 1: SWARM_E_BADARG; n_members > SWARM_PBT_MAX_MEMBERS:
 * SWARM_E_UNSUPPORTED; n_replace outside [0, n_members / 2]: SWARM_E_BADARG; unknown fields bits:
 * SWARM_E_BADARG; then SWARM_E_BADARG unless perturb_lo, perturb_hi are finite, > 0 and
 * lo <= hi, gamma_min <= gamma_max are finite, and 0 < lr_min <= lr_max are finite.
 * n_replace == 0 launches only the kernel that writes parent[m] = m.  Two launches otherwise, no
 * allocation, no host sync: capturable (round is a kernel argument: frozen into a hipGraph).
 * (tests/test_gpu_pop_pbt.py) */
#define SWARM_PBT_F_LR 1
#define SWARM_PBT_F_GAMMA 2
#define SWARM_PBT_MAX_MEMBERS 1024
typedef struct swarm_pbt_cfg {
  uint64_t seed;        /* Philox key of the PBT stream, split into k0/k1 as swarm_config.seed is */
  uint32_t round;       /* PBT round number: first counter word */
  int32_t n_replace;    /* members replaced = parents' pool size; 0 <= n_replace <= n_members / 2 */
  int32_t fields;       /* SWARM_PBT_F_*: which hyper-parameters a child perturbs */
  float perturb_lo, perturb_hi;       /* the two factors, e.g. 0.8f, 1.2f; finite, > 0 */
  float gamma_min, gamma_max;         /* clamp of the child's gamma */
  double lr_min, lr_max;              /* clamp of the child's lr_d */
} swarm_pbt_cfg;
int swarm_pop_exploit(const swarm_pbt_cfg* pbt, const float* score, swarm_adam_cfg* member_hp,
                      const swarm_pop_member* members, int32_t n_members, int32_t* parent, void* stream);

/* Workspace (floats) of swarm_td_grad's per-block gradient slabs. */
int64_t swarm_td_workspace_floats(const swarm_config* cfg, int32_t batch);

/* DQN TD-loss gradient (train_gcn_dqn.py:113-124): sample `batch` graphs from the
 * replay (keyed Philox permutation; or sample_in [batch] graph ids if non-NULL),
 * online forward, target forward + max, MSE, backward.  Writes per-block
 * gradient slabs (+ loss partial in column N_PARAMS) to `slabs`.
 * Skips (zero slabs, ctrl unchanged) while the replay holds < batch graphs. */
int swarm_td_grad(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* params,
                  const float* target, const swarm_replay* replay, const swarm_ctrl* ctrl,
                  const int32_t* sample_in, int32_t* sample_out, float* slabs, void* stream);

/* Deterministic fixed-order sum of the slabs -> grad[N_PARAMS + 1] (last = loss sum), plus the
 * clip norm's group partials at SWARM_GRAD_SQ_BASE (grad holds SWARM_GRAD_FLOATS floats). */
int swarm_grad_reduce(const swarm_config* cfg, const swarm_adam_cfg* hp, const float* slabs,
                      float* grad, void* stream);

/* clip_grad_norm_(1) + Adam step + target sync every `update_target_every` ticks,
 * then advance ctrl (tick, replay slot).  grad is the (all-reduced) gradient sum. */
int swarm_adam_step(const swarm_config* cfg, const swarm_adam_cfg* hp, float* params,
                    float* target, float* adam_m, float* adam_v, const float* grad,
                    int32_t replay_capacity, swarm_ctrl* ctrl, void* stream);

/* Initialise a control block: counters 0, eps, beta^0 = 1 and the Adam scalars of step 1. */
int swarm_ctrl_init(const swarm_adam_cfg* hp, float eps, swarm_ctrl* ctrl, void* stream);

/* Advance ctrl after an acting-only tick (no optimizer). */
int swarm_ctrl_advance(const swarm_config* cfg, const swarm_replay* replay, swarm_ctrl* ctrl, void* stream);

/* Host reference of the per-row neighbour selection the kernels run (CPU
 * torch.topk(largest=False) set semantics, libstdc++ introselect); for tests. */
int swarm_host_topk_set(const float* dist, int32_t n, int32_t k, uint8_t* selected);

#ifdef __cplusplus
}
#endif
#endif /* SWARM_HIP_H */
