"""swarm_pop_rollout: many policies rolled out by one launch, each bit for bit its lone swarm_rollout.

pop_rollout_kernel<NS, SCEN, SPEC, NET> (csrc/swarm_pop_rollout.hip) runs act_body of
act_kernel<NS, MODE_ROLLOUT, SCEN, SPEC, NET> for actor blockIdx.y, whose weights, state, outputs,
seed, tick0 and eps come from a descriptor in device memory; the dispatcher is launch_act's
(with_act_instance), so MATRIX of tests/test_gpu_rollout_matrix.py reaches its 37 instances too.
The reference side of every comparison is lone engines built fresh, never a population.

1. test_actors_equal_their_lone_rollouts_matrix: three actors per MATRIX row.
2. test_three_hundred_actors: grid.y = 300.
3. test_no_ticks_touch_nothing, test_actor_without_outputs: the C ABI directly.
4. test_captured_rollout_sees_a_rewritten_descriptor: hipGraph replays around a table rewrite.
5. test_population_simulator_writes_the_lone_simulators_files.
6. test_evaluation_during_training: SwarmPopulation.evaluate inside PopulationTrainer.
7. test_actor_population_refuses_what_one_launch_cannot_run.
"""
import contextlib
import ctypes
import io
import os

import pytest
import torch

from oracle import swarm_oracle as O
from tests.test_gpu_rollout_matrix import EPS, FL, G, MATRIX, _bits, _case_id, _start_state, _weights

pytestmark = pytest.mark.gpu

OUTPUTS = ("reward", "hits", "avg_dist", "obs", "traj_pos", "traj_dist", "traj_hits")
W_SEEDS, SEEDS, EPSS, TICK0S = (0, 3, 4), (4, 11, 4), (0.3, 0.0, 0.6), (7, 7, 1000)
B, T = 6, 6


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _engines(sw, golden_weights, case, n_envs, w_seeds, seeds):
    scen, N, graph, k, conv, net = case
    return [sw.SwarmEngine(scen, N, n_envs, seed=s, params=_weights(golden_weights, scen, net, w), graph=graph,
                           knn_k=max(k, 1), radius=0.3, conv=conv, net=net, learn=False, eps=EPS)
            for w, s in zip(w_seeds, seeds)]


def _assert_actor_is_lone(res, m, actor, lone, want, what):
    for k in OUTPUTS:
        assert _bits(res[k][m], want[k]), (what, m, k)
    assert _bits(actor.state, lone.state), (what, m, "state")
    if lone.scenario_state is not None:
        assert _bits(actor.scenario_state, lone.scenario_state), (what, m, "scenario_state")


# ------------------------------------------------------------------ 1. the kernel matrix
@pytest.mark.parametrize("case", MATRIX, ids=_case_id)
def test_actors_equal_their_lone_rollouts_matrix(sw, golden_weights, case):
    """Three actors (weights of model seeds 0, 3, 4; Philox seeds 4, 11, 4; eps 0.3, 0, 0.6; tick0
    7, 7, 1000) on 6 envs: two blocks per actor, the second with two dead waves."""
    acts = _engines(sw, golden_weights, case, B, W_SEEDS, SEEDS)
    lone = _engines(sw, golden_weights, case, B, W_SEEDS, SEEDS)
    pos, vel = _start_state(acts[0], lone[0], case, B)   # half reset grid, half in contact
    for e in acts[1:] + lone[1:]:
        e.set_state(pos, vel, fresh=True)
    res = sw.ActorPopulation(acts).rollout(T, tick0=TICK0S, eps=EPSS, traj=True)
    want = [e.rollout(T, tick0=t0, eps=eps, traj=True) for e, t0, eps in zip(lone, TICK0S, EPSS)]
    torch.cuda.synchronize()
    for m in range(3):
        _assert_actor_is_lone(res, m, acts[m], lone[m], want[m], _case_id(case))
    # actors 0 and 2 share the seed but not the weights or tick0: a kernel that read descriptor 0
    # for everyone would have passed for actor 0 only if they could not be told apart
    assert not _bits(want[0]["traj_pos"], want[2]["traj_pos"])
    assert res["traj_pos"].shape == (3, T, B, case[1], 2) and res["reward"].shape == (3, B, case[1])


# ------------------------------------------------------------------ 2. many actors
def test_three_hundred_actors(sw, golden_weights):
    case, P = (G, 5, "knn", 5, "gat", "gcn"), 300
    seeds = [1000 + 7 * m for m in range(P)]
    w_seeds = [m % 10 for m in range(P)]
    acts = _engines(sw, golden_weights, case, 1, w_seeds, seeds)
    for e in acts:
        e.reset(0)
    res = sw.ActorPopulation(acts).rollout(2, tick0=3, eps=0.5, traj=True)
    picks = (0, 137, 299)
    lone = _engines(sw, golden_weights, case, 1, [w_seeds[m] for m in picks], [seeds[m] for m in picks])
    want = []
    for e in lone:
        e.reset(0)
        want.append(e.rollout(2, tick0=3, eps=0.5, traj=True))
    torch.cuda.synchronize()
    for m, e, w in zip(picks, lone, want):
        _assert_actor_is_lone(res, m, acts[m], e, w, "300 actors")
    assert not _bits(want[0]["traj_pos"], want[2]["traj_pos"])


# ------------------------------------------------------------------ 3. nothing touched
def _table(L, rows, device):
    arr = (L.SwarmPopActor * len(rows))(*rows)
    raw = ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def _marked(N, n_envs, n_ticks, mark=12345.0):
    shapes = dict(reward=(n_envs, N), obs=(n_envs, N, 6), avg_dist=(n_envs,), hits=(n_envs,),
                  traj_pos=(n_ticks, n_envs, N, 2), traj_dist=(n_ticks, n_envs), traj_hits=(n_ticks, n_envs))
    return {k: torch.full(s, mark, device="cuda") for k, s in shapes.items()}


def _out_of(L, bufs):
    p = {k: v.data_ptr() for k, v in bufs.items()}
    return L.SwarmActOut(0, 0, p["reward"], p["obs"], p["avg_dist"], p["hits"], 0, p["traj_pos"], p["traj_dist"],
                         p["traj_hits"])


def test_no_ticks_touch_nothing(sw, golden_weights):
    from swarm_amd import _lib as L
    case = (G, 20, "knn", 5, "gat", "gcn")
    a, b = _engines(sw, golden_weights, case, B, (3, 3), (4, 4))
    _start_state(a, b, case, B)
    bufs = [_marked(case[1], B, 1), _marked(case[1], B, 1)]
    a2 = _engines(sw, golden_weights, case, B, (3,), (4,))[0]
    a2.state.copy_(a.state)
    rows = [L.SwarmPopActor(4, e.params.data_ptr(), e.state.data_ptr(), _out_of(L, bf), 7, EPS)
            for e, bf in zip((a, a2), bufs)]
    table = _table(L, rows, a.device)
    rc = a.lib.swarm_pop_rollout(ctypes.byref(a.cfg), table.data_ptr(), 2, 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert _bits(a.state, b.state) and _bits(a2.state, b.state)   # b never ran
    assert all(bool((v == 12345.0).all()) for bf in bufs for v in bf.values())


def test_actor_without_outputs(sw, golden_weights):
    """An actor whose out is all NULL beside one with every output set: the second is still exact,
    and the first's state advances as its lone rollout's does."""
    from swarm_amd import _lib as L
    case = (FL, 5, "knn", 5, "gat", "gcn")
    N = case[1]
    acts = _engines(sw, golden_weights, case, B, (0, 3), (4, 11))
    lone = _engines(sw, golden_weights, case, B, (0, 3), (4, 11))
    pos, vel = _start_state(acts[0], lone[0], case, B)
    for e in (acts[1], lone[1]):
        e.set_state(pos, vel, fresh=True)
    bufs = _marked(N, B, T)
    rows = [L.SwarmPopActor(4, acts[0].params.data_ptr(), acts[0].state.data_ptr(), L.SwarmActOut(), 7, 0.3),
            L.SwarmPopActor(11, acts[1].params.data_ptr(), acts[1].state.data_ptr(), _out_of(L, bufs), 9, 0.2)]
    table = _table(L, rows, acts[0].device)
    rc = acts[0].lib.swarm_pop_rollout(ctypes.byref(acts[0].cfg), table.data_ptr(), 2, T, L.stream_ptr())
    want = [lone[0].rollout(T, tick0=7, eps=0.3, traj=True), lone[1].rollout(T, tick0=9, eps=0.2, traj=True)]
    torch.cuda.synchronize()
    assert rc == 0
    for k in OUTPUTS:
        assert _bits(bufs[k], want[1][k]), k
    for m in range(2):
        assert _bits(acts[m].state, lone[m].state) and _bits(acts[m].scenario_state, lone[m].scenario_state), m
    assert not _bits(acts[0].state[..., :2], pos.to(acts[0].device))   # it moved


# ------------------------------------------------------------------ 4. a captured rollout
def test_captured_rollout_sees_a_rewritten_descriptor(sw, golden_weights):
    from swarm_amd.engine import capture_ticks
    case = (G, 8, "knn", 5, "gat", "gcn")
    acts = _engines(sw, golden_weights, case, B, W_SEEDS, SEEDS)
    lone = _engines(sw, golden_weights, case, B, W_SEEDS, SEEDS)
    pos, vel = _start_state(acts[0], lone[0], case, B)
    for e in acts[1:] + lone[1:]:
        e.set_state(pos, vel, fresh=True)
    start = [e._state_buf.clone() for e in acts]

    def restore():
        for e, l, s in zip(acts, lone, start):
            e._state_buf.copy_(s)
            l._state_buf.copy_(s)

    pop = sw.ActorPopulation(acts)
    args = dict(tick0=TICK0S, eps=EPSS, traj=True)
    pop.rollout(T, **args)    # writes the descriptor table; the captured call finds it current
    torch.cuda.synchronize()
    restore()
    graph = capture_ticks(acts[0].device, 1, lambda: pop.rollout(T, **args))
    torch.cuda.synchronize()
    assert all(_bits(e._state_buf, s) for e, s in zip(acts, start))   # a capture runs nothing
    res = pop.prepare(T, **args)   # the buffers the graph fills; no argument changed
    graph.replay()
    want = [e.rollout(T, tick0=t0, eps=eps, traj=True) for e, t0, eps in zip(lone, TICK0S, EPSS)]
    torch.cuda.synchronize()
    for m in range(3):
        _assert_actor_is_lone(res, m, acts[m], lone[m], want[m], "first replay")
    first = {k: v.clone() for k, v in res.items()}
    # actor 1: another tick0, eps and weights; the others keep theirs (in a table of new pointers)
    restore()
    tick0, eps = (7, 41, 1000), (0.3, 0.45, 0.6)
    new_w = torch.stack([_weights(golden_weights, G, "gcn", w) for w in (0, 7, 4)]).to(acts[0].device)
    assert pop.prepare(T, tick0=tick0, eps=eps, traj=True, params=new_w) is res
    graph.replay()
    want = [e.rollout(T, tick0=t0, eps=ep, traj=True, params=new_w[m])
            for m, (e, t0, ep) in enumerate(zip(lone, tick0, eps))]
    torch.cuda.synchronize()
    for m in range(3):
        _assert_actor_is_lone(res, m, acts[m], lone[m], want[m], "second replay")
    assert _bits(res["traj_pos"][0], first["traj_pos"][0]) and _bits(res["traj_pos"][2], first["traj_pos"][2])
    assert not _bits(res["traj_pos"][1], first["traj_pos"][1])


# ------------------------------------------------------------------ 5. PopulationSimulator
def _sim_env(sw, scen_cls):
    return sw.make_env(getattr(sw, scen_cls)(), scenario_name="test_gcn_vmas", num_envs=1, continuous_actions=False,
                       dict_spaces=True, wrapper=None, seed=6967, n_agents=5, max_steps=10, random=True)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("scen_cls,net", [("GoToPositionScenario", "gcn"), ("FlockingScenario", "gat3")])
def test_population_simulator_writes_the_lone_simulators_files(sw, golden_weights, tmp_path, scen_cls, net):
    def model(seed):
        if net == "gat3":
            return sw.GCN.from_state_dict(O.gat3_unflatten(torch.tensor(golden_weights["flocking_gat3"][seed])))
        m = sw.GCN(7, 32, 9)
        # the trained GoTo policies all head straight for the goal (identical 10-tick files), so
        # the third model is an untrained one
        w = (torch.tensor(golden_weights["go_to"][seed]) if seed != 4
             else sw.engine.glorot_init(torch.Generator().manual_seed(seed)))
        m.load_state_dict(O.unflatten_params(w))
        return m
    seeds = (0, 3, 4)
    pop_dirs = [str(tmp_path / "pop" / f"seed_{s}") for s in seeds]
    lone_dirs = [str(tmp_path / "lone" / f"seed_{s}") for s in seeds]
    with contextlib.redirect_stdout(io.StringIO()):
        sw.PopulationSimulator(_sim_env(sw, scen_cls), [model(s) for s in seeds], 2, "test", 6967, pop_dirs,
                               knn_k=5).run_simulation()
        for s, d in zip(seeds, lone_dirs):
            sw.Simulator(_sim_env(sw, scen_cls), model(s), 2, "test", 6967, output_dir=d, knn_k=5).run_simulation()
    per_seed = []
    for pd, ld in zip(pop_dirs, lone_dirs):
        got, want = _files(pd), _files(ld)
        assert sorted(got) == sorted(want) and len(want) == 1 + 2 * 2 + 2   # result, x / y per episode, distances
        for name in want:
            assert got[name] == want[name], (pd, name)
        per_seed.append(tuple(want[n] for n in sorted(want)))
    assert len(set(per_seed)) > 1   # the models do differ


# ------------------------------------------------------------------ 6. evaluation during training
def _trainer(sw, seed, root):
    env = sw.make_env(scenario=sw.GoToPositionScenario(), num_envs=1, continuous_actions=False, wrapper=None,
                      max_steps=10, dict_spaces=True, n_agents=5, seed=seed)
    sw.set_seed(seed)
    return sw.DQNTrainer(env, seed, os.path.join(root, "models"), os.path.join(root, "stats"), "GoTo", batch_size=4,
                         replay_capacity=1000)


def test_evaluation_during_training(sw, tmp_path):
    config = {"epsilon": 0.99, "epsilon_decay": 0.01, "min_epsilon": 0.05, "episodes": 3}
    with_eval = dict(config, eval_every=1, eval_envs=3)
    seeds = (0, 1)
    runs = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for name, cfg in (("eval", with_eval), ("plain", config)):
            runs[name] = [_trainer(sw, s, str(tmp_path / name)) for s in seeds]
            sw.PopulationTrainer(runs[name]).train_model(cfg)
        runs["lone"] = [_trainer(sw, s, str(tmp_path / "lone")) for s in seeds]
        for t in runs["lone"]:
            t.train_model(with_eval)
    torch.cuda.synchronize()
    # evaluation leaves the training run every bit: weights, moments, target, ring, state, control block
    for a, b in zip(runs["eval"], runs["plain"]):
        ea, eb = a.engine, b.engine
        for k in ("_lrn", "grad", "rep_s", "rep_s1", "rep_r", "rep_a", "_state_buf", "ctrl", "samples"):
            assert torch.equal(getattr(ea, k), getattr(eb, k)), k
        assert b.eval_rows == [] and not os.path.exists(os.path.join(b.stats_path, "experiment_GoTo-seed_0-eval.csv"))
    # each member's rows are its lone trainer's
    for a, l in zip(runs["eval"], runs["lone"]):
        assert torch.equal(a.engine._lrn, l.engine._lrn)
        assert [r[0] for r in a.eval_rows] == [0, 1, 2]
        assert a.eval_rows == l.eval_rows, (a.eval_rows, l.eval_rows)
        assert all(len(r) == 4 and all(x == x for x in r) for r in a.eval_rows)
        name = f"experiment_GoTo-seed_{a.seed}-eval.csv"
        ca = open(os.path.join(a.stats_path, name), "rb").read()
        assert ca == open(os.path.join(l.stats_path, name), "rb").read()
        assert ca.startswith(b"Episode,Reward,Collisions,Distance (end)") and ca.count(b"\n") == 4
    assert runs["eval"][0].eval_rows != runs["eval"][1].eval_rows   # two policies, one set of envs


# ------------------------------------------------------------------ 7. ActorPopulation's checks
def test_actor_population_refuses_what_one_launch_cannot_run(sw, golden_weights):
    case = (G, 5, "knn", 5, "gat", "gcn")
    a, b = _engines(sw, golden_weights, case, 2, (0, 3), (4, 11))
    with pytest.raises(ValueError):
        sw.ActorPopulation([a, _engines(sw, golden_weights, (G, 8, "knn", 5, "gat", "gcn"), 2, (0,), (4,))[0]])
    with pytest.raises(ValueError):
        sw.ActorPopulation([a, _engines(sw, golden_weights, (G, 5, "complete", 0, "gat", "gcn"), 2, (0,), (4,))[0]])
    with pytest.raises(ValueError):
        sw.ActorPopulation([])
    pop = sw.ActorPopulation([a, b])
    with pytest.raises(ValueError):
        pop.rollout(2, tick0=[1, 2, 3])
    with pytest.raises(ValueError):
        pop.rollout(2, eps=[0.1])
    with pytest.raises(ValueError):
        pop.rollout(2, params=torch.zeros(3, a.params.numel(), device=a.device))
