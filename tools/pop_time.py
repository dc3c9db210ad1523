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

usage: python tools/pop_time.py [--rollout] [--repeats 7] [--sizes 1,10,64] [--out population_time.json]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rollout", action="store_true", help="time evaluation rollouts instead of training ticks")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1,10,64")
    ap.add_argument("--configs", default=None, help="e.g. GoTo:5,ObstacleAvoidance:10 (default: all four)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    configs = CONFIGS if not a.configs else tuple((c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(","))
    rows = []
    for scen, N in configs:
        for P in [int(x) for x in a.sizes.split(",")]:
            rows.append((measure_rollout if a.rollout else measure)(scen, N, P, a.repeats))
            print(json.dumps(rows[-1]), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
