// swarm_launch.h — host side of libswarm_hip.so between the C ABI and hipLaunchKernelGGL (host
// only; swarm_act.hip, swarm_td.hip, swarm_tick.hip): the config check, the kernel argument blocks,
// the TD grid, and the dispatcher from runtime (N, scenario, net, graph / conv) to one kernel.
#pragma once
#include <type_traits>

#include "swarm_actk.h"
#include "swarm_tdk.h"

namespace swarm {

// ---- config check: what differs between the entry points; the rest is shared
struct CfgRules {
  int max_agents;     // 32; 16 for the fused tick
  bool dense_ok;      // SWARM_GRAPH_DENSE (a caller-supplied multiplicity) is accepted
  bool empty_ok;      // n_envs == 0 is a valid no-op
  bool env_checked;   // scenario and conv are validated (the TD side has always taken them as given)
  bool learner;       // any net but the GCN is SWARM_E_UNSUPPORTED (GAT3 has entry points of its own: swarm_gat3_*)
  bool hp_checked;    // hp is required: batch first, world_size / update_target_every last of all
};
constexpr CfgRules kCfgAct = {32, true, true, true, false, false};        // acting / env entry points
constexpr CfgRules kCfgActGraph = {32, false, true, true, false, false};  // ... that build the graph themselves
constexpr CfgRules kCfgTd = {32, false, false, false, true, true};        // TD, reduce, Adam entry points
constexpr CfgRules kCfgTick = {16, false, false, true, true, false};      // swarm_train_tick
constexpr CfgRules kCfgQBackward = {32, true, false, true, true, false};  // swarm_q_backward: kCfgAct for a learner
constexpr CfgRules kCfgGat3Backward = {32, true, false, true, false, false};   // swarm_gat3_q_backward: kCfgAct, n_envs >= 1
// swarm_gat3_td_grad / swarm_gat3_adam_step: kCfgTd with the net rule turned round (the entry points refuse the
// GCN themselves, then world_size != 1, and only then the dense graph)
constexpr CfgRules kCfgGat3Td = {32, true, false, false, false, true};
// 0 or the first error, in the order the entry points have always reported them (tests/test_cpu_host.py)
inline int check_config(const swarm_config* c, const CfgRules& r, const swarm_adam_cfg* hp = nullptr) {
  if (!c || c->n_agents < 1 || c->n_agents > r.max_agents || c->n_envs < (r.empty_ok ? 0 : 1)) return SWARM_E_BADARG;
  if (r.hp_checked && (!hp || hp->batch < 1)) return SWARM_E_BADARG;
  if (c->graph < 0 || c->graph > 3 || (c->graph == SWARM_GRAPH_DENSE && !r.dense_ok)) return SWARM_E_BADARG;
  if (r.env_checked) {
    if (c->scenario != SWARM_GOTO && c->scenario != SWARM_OBSTACLE_AVOIDANCE && c->scenario != SWARM_FLOCKING)
      return SWARM_E_BADARG;
    if (c->scenario == SWARM_FLOCKING && c->n_agents < 2) return SWARM_E_BADARG;   // mean over the other agents
    if (c->conv != SWARM_CONV_GAT && c->conv != SWARM_CONV_GCN) return SWARM_E_BADARG;
  }
  if (r.learner && c->net != SWARM_NET_GCN) return SWARM_E_UNSUPPORTED;
  if (c->net != SWARM_NET_GCN && (c->net != SWARM_NET_GAT3 || c->conv != SWARM_CONV_GAT)) return SWARM_E_BADARG;
  if (c->graph == SWARM_GRAPH_KNN && (c->knn_k < 1 || c->knn_k > c->n_agents)) return SWARM_E_KNN_K;
  if (c->graph == SWARM_GRAPH_RADIUS && !(c->radius > 0.0f)) return SWARM_E_BADARG;
  if (r.hp_checked && (hp->world_size < 1 || hp->update_target_every < 1)) return SWARM_E_BADARG;
  return 0;
}

// ---- kernel argument blocks
inline uint32_t seed_k0(const swarm_config* c) { return (uint32_t)(c->seed & 0xFFFFFFFFu); }
inline uint32_t seed_k1(const swarm_config* c) { return (uint32_t)(c->seed >> 32); }
// slots of a TD graph of N agents, and of the wave that runs it (two 8-slot graphs share 16 slots)
constexpr int td_slots(int n_agents) { return n_agents <= 8 ? 8 : (n_agents <= 16 ? 16 : 32); }
constexpr int td_wave_slots(int gs) { return gs < 16 ? 16 : gs; }
// TD blocks (= gradient slabs) of a batch, in td_kernel and in the fused tick alike: 32 / GS graphs each
inline int td_blocks(int n_agents, int batch) {
  const int gpb = kTdRows / td_slots(n_agents);
  return (batch + gpb - 1) / gpb;
}

inline ActArgs make_act_args(const swarm_config* c) {
  ActArgs a = {};
  a.B = c->n_envs; a.N = c->n_agents; a.scenario = c->scenario; a.graph = c->graph;
  a.k = c->knn_k; a.conv = c->conv; a.env_offset = c->env_offset; a.flags = c->flags;
  a.k0 = seed_k0(c); a.k1 = seed_k1(c); a.radius = c->radius; a.net = c->net;
  return a;
}

inline TdArgs make_td_args(const swarm_config* c, const swarm_adam_cfg* hp, const float* params, const float* target,
                           const swarm_replay* replay, const swarm_ctrl* ctrl, const int32_t* sample_in,
                           int32_t* sample_out, float* slabs) {
  TdArgs a = {};
  a.S = hp->batch; a.B = c->n_envs; a.N = c->n_agents; a.graph = c->graph; a.k = c->knn_k;
  a.conv = c->conv; a.env_offset = c->env_offset;
  a.k0 = seed_k0(c); a.k1 = seed_k1(c); a.radius = c->radius;
  a.params = params; a.target = target; a.replay = *replay; a.ctrl = ctrl;
  a.sample_in = sample_in; a.sample_out = sample_out; a.slabs = slabs;
  a.gamma = hp->gamma;
  a.grad_scale = (float)(2.0 / ((double)hp->batch * (double)c->n_agents));   // MSELoss mean over the batch nodes
  a.n_slabs = td_blocks(c->n_agents, hp->batch);
  return a;
}

// ---- dispatcher: with_* turn a runtime value into a std::integral_constant and call f with it; a
// launch nests them and names its kernel once, in the innermost generic lambda.  What a rule does
// not allow is cut with `if constexpr`, so the rules are also the list of kernels that exist.
template <int V>
using ic = std::integral_constant<int, V>;
// the smallest of the ascending slot counts that holds n; the last takes the rest
template <int V, int... Vs, class F>
void with_slots(int n, F&& f) {
  if constexpr (sizeof...(Vs) > 0) {
    if (n > V) return with_slots<Vs...>(n, f);
  }
  f(ic<V>{});
}
// the V of V, Vs... that equals v and that Rule::allows; D otherwise
template <class Rule, int D, int V, int... Vs, class F>
void with_choice(int v, F&& f) {
  if constexpr (Rule::allows(V)) {
    if (v == V) return f(ic<V>{});
  }
  if constexpr (sizeof...(Vs) > 0) with_choice<Rule, D, Vs...>(v, f);
  else f(ic<D>{});
}
template <bool OK>
struct AllIf { static constexpr bool allows(int) { return OK; } };
// scenario (validated by check_config); PHYSICS = false (MODE_Q: no env step) folds all into GoTo
template <bool PHYSICS = true, class F>
void with_scenario(int scenario, F&& f) {
  with_choice<AllIf<PHYSICS>, SWARM_GOTO, SWARM_OBSTACLE_AVOIDANCE, SWARM_FLOCKING>(scenario, f);
}
// net; FORWARD = false (MODE_STEP: no network runs) has the GCN kernels only
template <bool FORWARD, class F>
void with_net(int net, F&& f) { with_choice<AllIf<FORWARD>, SWARM_NET_GCN, SWARM_NET_GAT3>(net, f); }
// graph / conv specialisation where Rule::allows it, else SPEC_RUNTIME (same numbers, slower)
template <class Rule, class F>
void with_spec(int graph, int conv, F&& f) {
  with_choice<Rule, SPEC_RUNTIME, SPEC_COMPLETE_GAT, SPEC_COMPLETE_GCN, SPEC_KNN_GAT, SPEC_RADIUS_GAT>(
      spec_of(graph, conv), f);
}

// ---- the kernel families' rules: which SPEC_* each has
constexpr bool spec_complete(int sp) { return sp == SPEC_COMPLETE_GAT || sp == SPEC_COMPLETE_GCN; }
// SPEC_RADIUS_GAT (the north_star graph) is built for GoTo with <= 8 slots only
constexpr bool spec_radius_gat(int sp, int ns, int scen) {
  return sp == SPEC_RADIUS_GAT && ns == 8 && scen == SWARM_GOTO;
}
// act_kernel<NS, MODE, SCEN, SPEC, NET>: MODE_Q, MODE_STEP, Flocking and the three-layer GAT have
// SPEC_RUNTIME only; the tick has the complete graph; the rollout adds kNN + GAT and radius + GAT
template <int NS, int MODE, int SCEN, int NET>
struct ActSpecs {
  static constexpr bool allows(int sp) {
    if (SCEN == SWARM_FLOCKING || NET != SWARM_NET_GCN) return false;
    if (MODE == MODE_ROLLOUT) return spec_complete(sp) || sp == SPEC_KNN_GAT || spec_radius_gat(sp, NS, SCEN);
    return MODE == MODE_TICK && spec_complete(sp);
  }
};
// (N, scenario, net, graph, conv) -> f(NS, SCEN, NET, SPEC) of the act_kernel instance of MODE
// (ActSpecs); launch_act (swarm_act.hip) and the population rollout (swarm_pop_rollout.hip), whose
// kernel template takes <NS, SCEN, SPEC, NET> for MODE_ROLLOUT, name their kernels through it
template <int MODE, class F>
void with_act_instance(const ActArgs& a, F&& f) {
  with_slots<8, 16, 32>(a.N, [&](auto ns) {
    with_scenario<MODE != MODE_Q>(a.scenario, [&](auto sc) {
      with_net<MODE != MODE_STEP>(a.net, [&](auto net) {
        with_spec<ActSpecs<decltype(ns)::value, MODE, decltype(sc)::value, decltype(net)::value>>(
            a.graph, a.conv, [&](auto sp) { f(ns, sc, net, sp); });
      });
    });
  });
}
// tick_kernel<NSA = 8 or 16, td_wave_slots(NSA), NSA, SCEN, SPEC>: the complete graph, radius + GAT
template <int NSA, int SCEN>
struct TickSpecs {
  static constexpr bool allows(int sp) { return spec_complete(sp) || spec_radius_gat(sp, NSA, SCEN); }
};
// td_kernel<td_wave_slots(GS), GS, SPEC>: the complete graph, the reference's training graph
struct TdSpecs {
  static constexpr bool allows(int sp) { return spec_complete(sp); }
};

// ---- the fused tick's launch (tick_kernel in swarm_tick.hip; pop_tick_kernel, one learner per
// blockIdx.y, in swarm_pop.hip)
// workspace: [err: 1 u32, padded to kTickErrBytes], then the tagged hand-off records
constexpr int kTickErrBytes = 512;
// the grid's x extent: acting blocks first, then one TD block per slab
inline int tick_grid_x(int n_envs, int n_slabs) { return (n_envs + kActWPB - 1) / kActWPB + n_slabs; }
// (N, scenario, graph, conv) -> f(NSA, SCEN, SPEC) of the tick instance (TickSpecs); the caller's
// kernel template takes <NSA, td_wave_slots(NSA), NSA, SCEN, SPEC>
template <class F>
void with_tick_instance(const swarm_config* c, F&& f) {
  with_slots<8, 16>(c->n_agents, [&](auto ns) {
    with_scenario(c->scenario, [&](auto sc) {
      with_spec<TickSpecs<decltype(ns)::value, decltype(sc)::value>>(c->graph, c->conv,
                                                                     [&](auto sp) { f(ns, sc, sp); });
    });
  });
}

}  // namespace swarm
