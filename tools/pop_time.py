"""Time a population tick against the same work done one learner at a time.

At the reference's shape (src/training/train_gcn_dqn.py:262-290: 1 env, batch 32, the default
ring, 100-tick episodes) and P learners (seeds 0..P-1), two ways of running one episode of all P:
  sequential : P lone SwarmEngines, each replaying its own captured 100-tick episode (hipGraph),
               one after another on one stream: what running the seeds in turn costs;
  population : one SwarmPopulation replaying one captured 100-tick episode of all P members;
  population_hp : the same with one optimizer row per member (swarm_pop_train_tick_hp /
               swarm_pop_reduce_advance_hp): the members get distinct lr and gamma values.
All are timed between two HIP events around `K` back-to-back episode replays (no host
synchronisation inside), after a warm-up of all that also fills the replay rings past the batch
size, so every timed tick trains.  The ways alternate, `--repeats` times each; the table gives the
median and the spread in us per population tick (= one tick of all P learners).  Environment
resets are not timed (they are per-member launches in both).

``--rollout`` times evaluation instead, at the evaluation shape (kNN-5 graph, 8 envs, 100 greedy
ticks, P policies = model seeds 0..P-1 of random weights on the same starts):
  sequential : P lone swarm_rollout launches one after another on one stream (captured once into
               one hipGraph, so no host time is between them): what evaluating the policies in turn costs;
  population : one swarm_pop_rollout launch of all P (captured likewise).
Same method: HIP events around back-to-back replays, the ways alternating, medians with min and
max, here in us per evaluation of all P policies (one 100-tick rollout each).  The states are not
reset between replays (both ways advance theirs alike).

``--pbt`` times one round of population-based training at the reference's shape (1 env, batch 32),
P learners that have trained for 40 ticks, frac = 0.25, lr and gamma perturbed, a fixed device score:
  exploit_graph : `rounds` calls of SwarmPopulation.exploit(sync=False) (swarm_pop_exploit: the plan
               and the copy launch, nothing read back) captured into one hipGraph, replayed: the
               device time of a round;
  exploit_eager : the same calls issued eagerly, back to back: what a round costs a Python caller;
  host        : the same round done with what the population offered before swarm_pop_exploit: a
               host read of the scores, the ranking on the host, per replaced member tensor copies
               of the same buffers (seven learner rows, grad, the optimizer's control words) and a
               set_member_hp.
Same method: HIP events around back-to-back rounds, the ways alternating, medians with min and max,
in us per round.  Default sizes 10,64.

``--gat3`` times the three-layer GAT's learners at the reference's Flocking shape (10 agents, 1 env,
batch 32, the default ring, 100-tick episodes), P learners (seeds 0..P-1):
  sequential : P lone SwarmGat3Engines, each replaying its own captured 100-tick episode (4 launches
               per tick), one after another on one stream;
  population : one SwarmGat3Population replaying one captured 100-tick episode of all P members (the
               same 4 launches per tick, the member as the grid's second dimension).
Same method as the default mode; us per population tick.  Default output profiles/gat3_pop_time.json.

usage: python tools/pop_time.py [--rollout | --pbt | --gat3] [--repeats 7] [--sizes 1,10,64] [--out population_time.json]
Prints one JSON line per configuration and population size.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swarm_amd  # noqa: E402
import swarm_amd._lib as L  # noqa: E402

CONFIGS = (("GoTo", 5), ("GoTo", 10), ("ObstacleAvoidance", 5), ("ObstacleAvoidance", 10))
TICKS = 100


def window_us(replay, episodes):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(episodes):
        replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (episodes * TICKS)


def measure(scen, N, P, repeats):
    kw = dict(scenario=scen, n_agents=N, n_envs=1, batch=32, eps=0.05, shared_reset=True)
    lone = [swarm_amd.SwarmEngine(seed=s, **kw) for s in range(P)]
    pop = swarm_amd.SwarmPopulation(seeds=list(range(P)), **kw)
    # a sweep: every member its own lr and gamma; P = 1 has one row, so the _hp pair is forced
    sweep = dict(lr=[1e-3 / (1 + m / 8) for m in range(P)], gamma=[0.99 - 0.25 * m / P for m in range(P)])
    pop_hp = swarm_amd.SwarmPopulation(seeds=list(range(P)), **sweep, **kw)
    pop_hp.per_member_hp = True
    assert not pop.per_member_hp
    for e in lone:
        e.reset(0)
    pop.reset(0)
    pop_hp.reset(0)
    lone_graphs = [e.capture(TICKS) for e in lone]
    pop_graph = pop.capture(TICKS)
    pop_hp_graph = pop_hp.capture(TICKS)

    def sequential():
        for g in lone_graphs:
            g.replay()

    ways = {"sequential": sequential, "population": pop_graph.replay, "population_hp": pop_hp_graph.replay}
    # enough episodes per window that it lasts tens of milliseconds at least
    episodes = {"sequential": max(2, math.ceil(40 / P)), "population": 40, "population_hp": 40}
    for k, fn in ways.items():   # warm-up: code objects loaded, rings past the batch size, clocks up
        window_us(fn, 2)
    times = {k: [] for k in ways}
    for _ in range(repeats):
        for k, fn in ways.items():
            times[k].append(window_us(fn, episodes[k]))
    torch.cuda.synchronize()
    pop.check_handoffs()
    pop_hp.check_handoffs()
    for e in lone:
        e.check_handoffs()
    steps = [c["adam_step"] for c in pop.read_ctrl() + pop_hp.read_ctrl()]
    assert min(steps) > 0, "the timed ticks did not train"
    out = {"scenario": scen, "n_agents": N, "n_envs": 1, "batch": 32, "population": P, "ticks_per_episode": TICKS,
           "episodes_per_window": episodes, "repeats": repeats, "build": pop.lib.swarm_build_info().decode()}
    for k, v in times.items():
        out[k + "_us_per_tick"] = round(statistics.median(v), 3)
        out[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    out["sequential_over_population"] = round(out["sequential_us_per_tick"] / out["population_us_per_tick"], 3)
    out["population_hp_over_population"] = round(out["population_hp_us_per_tick"] / out["population_us_per_tick"], 4)
    return out


def measure_rollout(scen, N, P, repeats, n_envs=8, knn_k=5):
    kw = dict(scenario=scen, n_agents=N, n_envs=n_envs, graph="knn", knn_k=knn_k, learn=False, eps=0.0)
    gen = torch.Generator().manual_seed(1234)
    weights = [swarm_amd.engine.glorot_init(gen) for _ in range(P)]
    lone = [swarm_amd.SwarmEngine(seed=6967, params=w, **kw) for w in weights]
    acts = [swarm_amd.SwarmEngine(seed=6967, params=w, **kw) for w in weights]
    for e in lone + acts:
        e.reset(0)
    pop = swarm_amd.ActorPopulation(acts)
    pop.rollout(TICKS)   # writes the descriptor table; the captured call below finds it current
    outs = [(e, torch.zeros(n_envs, N, device=e.device), torch.zeros(n_envs, device=e.device),
             torch.zeros(n_envs, device=e.device)) for e in lone]

    def sequential():   # what SwarmEngine.rollout launches, without its allocations
        for e, rew, dist, hits in outs:
            out = L.SwarmActOut(0, 0, rew.data_ptr(), 0, dist.data_ptr(), hits.data_ptr(), 0, 0, 0, 0)
            L.call(e.lib, "swarm_rollout", e.cfg, e.params.data_ptr(), e.state.data_ptr(), TICKS, 0, 0.0, out)

    dev = lone[0].device
    graphs = {"sequential": swarm_amd.engine.capture_ticks(dev, 1, sequential),
              "population": swarm_amd.engine.capture_ticks(dev, 1, lambda: pop.rollout(TICKS))}
    # enough replays per window that it lasts tens of milliseconds at least
    reps = {"sequential": max(4, math.ceil(200 / P)), "population": 200}

    def window(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps[k]):
            graphs[k].replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps[k]

    for k in graphs:
        window(k)
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for k in graphs:
            times[k].append(window(k))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(e.state).all()) for e in lone + acts)
    out = {"mode": "rollout", "scenario": scen, "n_agents": N, "n_envs": n_envs, "graph": f"knn{knn_k}", "population": P,
           "ticks": TICKS, "replays_per_window": reps, "repeats": repeats,
           "build": lone[0].lib.swarm_build_info().decode()}
    for k, v in times.items():
        out[k + "_us"] = round(statistics.median(v), 3)
        out[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    out["sequential_over_population"] = round(out["sequential_us"] / out["population_us"], 3)
    out["slowest_population_beats_fastest_sequential"] = max(times["population"]) < min(times["sequential"])
    return out


def measure_gat3(scen, N, P, repeats):
    kw = dict(scenario=scen, n_agents=N, n_envs=1, batch=32, eps=0.05, shared_reset=True)
    lone = [swarm_amd.SwarmGat3Engine(seed=s, **kw) for s in range(P)]
    pop = swarm_amd.SwarmGat3Population(seeds=list(range(P)), **kw)
    assert not pop.per_member_hp
    for e in lone:
        e.reset(0)
    pop.reset(0)
    lone_graphs = [e.capture(TICKS) for e in lone]
    pop_graph = pop.capture(TICKS)

    def sequential():
        for g in lone_graphs:
            g.replay()

    ways = {"sequential": sequential, "population": pop_graph.replay}
    # enough episodes per window that it lasts tens of milliseconds at least
    episodes = {"sequential": max(2, math.ceil(40 / P)), "population": 40}
    for k, fn in ways.items():   # warm-up: code objects loaded, rings past the batch size, clocks up
        window_us(fn, 2)
    times = {k: [] for k in ways}
    for _ in range(repeats):
        for k, fn in ways.items():
            times[k].append(window_us(fn, episodes[k]))
    torch.cuda.synchronize()
    ctrl = pop.read_ctrl() + [e.read_ctrl() for e in lone]
    assert min(c["adam_step"] for c in ctrl) > 0, "the timed ticks did not train"
    assert all(math.isfinite(c["loss"]) for c in ctrl)
    out = {"mode": "gat3", "scenario": scen, "n_agents": N, "n_envs": 1, "batch": 32, "population": P,
           "ticks_per_episode": TICKS, "launches_per_tick": {"sequential": 4 * P, "population": 4},
           "episodes_per_window": episodes, "repeats": repeats, "build": pop.lib.swarm_build_info().decode()}
    for k, v in times.items():
        out[k + "_us_per_tick"] = round(statistics.median(v), 3)
        out[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    out["sequential_over_population"] = round(out["sequential_us_per_tick"] / out["population_us_per_tick"], 3)
    out["slowest_population_beats_fastest_sequential"] = max(times["population"]) < min(times["sequential"])
    return out


PBT_ROUNDS = 50
PBT_CTRL_WORDS = [3, 5, 6, 7, 10, 11, 12, 13, 14, 15, 24, 25]   # what swarm_pop_exploit copies of swarm_ctrl


def measure_pbt(scen, N, P, repeats):
    kw = dict(scenario=scen, n_agents=N, n_envs=1, batch=32, eps=0.05, shared_reset=True)
    pops = {}
    for way in ("exploit_graph", "exploit_eager", "host"):
        pop = pops[way] = swarm_amd.SwarmPopulation(seeds=list(range(P)), **kw)
        pop.per_member_hp = True
        pop.reset(0)
        for _ in range(40):   # past the batch size: moments, a pending step
            pop.train_tick()
    dev = pops["host"].device
    score = torch.randn(P, generator=torch.Generator().manual_seed(5)).to(dev)
    pbt = dict(frac=0.25, fields=("lr", "gamma"), seed=1)
    n_replace = int(pbt["frac"] * P)

    def device_rounds(pop):
        for r in range(PBT_ROUNDS):
            pop.exploit(score, round=r, sync=False, **pbt)

    def host_round(pop, r):
        s = score.tolist()   # the host read
        order = sorted(range(P), key=lambda m: (-s[m], m))
        for i, c in enumerate(order[P - n_replace:]):
            p = order[(i + r) % n_replace]
            ce, pe = pop.members[c], pop.members[p]
            ce._lrn[:, :L.N_PARAMS].copy_(pe._lrn[:, :L.N_PARAMS])
            ce.grad.copy_(pe.grad)
            ce.ctrl[PBT_CTRL_WORDS] = pe.ctrl[PBT_CTRL_WORDS]
            f = 0.8 if (i + r) % 2 else 1.2
            pop.set_member_hp(c, lr=min(max(pe.hp.lr_d * f, 1e-6), 1e-1),
                              gamma=min(max(1.0 - (1.0 - pe.hp.gamma) * f, 0.0), 0.9999),
                              betas=(pe.hp.beta1_d, pe.hp.beta2_d), adam_eps=pe.hp.eps, max_norm=pe.hp.max_norm,
                              update_target_every=pe.hp.update_target_every)

    def host_rounds():
        for r in range(PBT_ROUNDS):
            host_round(pops["host"], r)

    graph = swarm_amd.engine.capture_ticks(dev, 1, lambda: device_rounds(pops["exploit_graph"]))
    ways = {"exploit_graph": graph.replay, "exploit_eager": lambda: device_rounds(pops["exploit_eager"]),
            "host": host_rounds}
    # chains of PBT_ROUNDS rounds per window: enough that a window lasts tens of milliseconds
    windows = {"exploit_graph": 200, "exploit_eager": 50, "host": max(1, 40 // P)}

    def window(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(windows[k]):
            ways[k]()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / (windows[k] * PBT_ROUNDS)

    for k in ways:
        window(k)
    times = {k: [] for k in ways}
    for _ in range(repeats):
        for k in ways:
            times[k].append(window(k))
    torch.cuda.synchronize()
    for pop in pops.values():   # the populations still train after all those rounds
        pop.sync_hp()
        pop.train_tick()
        pop.check_handoffs()
        assert all(math.isfinite(c["loss"]) for c in pop.read_ctrl())
    assert int((pops["exploit_graph"].parent != torch.arange(P, device=dev)).sum()) == n_replace
    out = {"mode": "pbt", "scenario": scen, "n_agents": N, "n_envs": 1, "batch": 32, "population": P,
           "n_replace": n_replace, "rounds_per_chain": PBT_ROUNDS, "chains_per_window": windows, "repeats": repeats,
           "build": pops["host"].lib.swarm_build_info().decode()}
    for k, v in times.items():
        out[k + "_us_per_round"] = round(statistics.median(v), 3)
        out[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    out["host_over_exploit_eager"] = round(out["host_us_per_round"] / out["exploit_eager_us_per_round"], 2)
    out["host_over_exploit_graph"] = round(out["host_us_per_round"] / out["exploit_graph_us_per_round"], 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rollout", action="store_true", help="time evaluation rollouts instead of training ticks")
    ap.add_argument("--pbt", action="store_true", help="time one PBT round: swarm_pop_exploit against host copies")
    ap.add_argument("--gat3", action="store_true", help="time SwarmGat3Population against lone SwarmGat3Engines")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default=None, help="population sizes (default 1,10,64; --pbt: 10,64)")
    ap.add_argument("--configs", default=None, help="e.g. GoTo:5,ObstacleAvoidance:10 (default: all four)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.sizes = a.sizes or ("10,64" if a.pbt else "1,10,64")
    if a.pbt and not a.configs:
        a.configs = "GoTo:5"
    if a.gat3:
        a.configs = a.configs or "Flocking:10"
        a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                      "gat3_pop_time.json")
    fn = measure_gat3 if a.gat3 else measure_pbt if a.pbt else measure_rollout if a.rollout else measure
    configs = CONFIGS if not a.configs else tuple((c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(","))
    rows = []
    for scen, N in configs:
        for P in [int(x) for x in a.sizes.split(",")]:
            rows.append(fn(scen, N, P, a.repeats))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
