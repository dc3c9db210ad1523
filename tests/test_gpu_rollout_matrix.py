"""swarm_rollout across its kernel matrix, with exploration, a non-zero first tick, 17-32 agents,
dead waves and a shard offset.

launch_act<MODE_ROLLOUT> (csrc/swarm_act.hip) picks one act_kernel<NS, MODE_ROLLOUT, SCEN, SPEC, NET>
by slots NS (8 / 16 / 32 for up to 8 / 16 / 32 agents), scenario, net and, where ActSpecs
(csrc/swarm_launch.h) has it, a graph / conv specialisation:

    net GCN, GoTo or OA   SPEC_COMPLETE_GAT, SPEC_COMPLETE_GCN, SPEC_KNN_GAT, SPEC_RUNTIME (kNN + GCNConv,
                          radius + GCNConv, radius + GAT) at every NS                    2 x 3 x 4 = 24
    net GCN, GoTo, NS 8   SPEC_RADIUS_GAT (radius + GAT is SPEC_RUNTIME everywhere else)              1
    net GCN, Flocking     SPEC_RUNTIME at every NS                                                    3
    net GAT3              SPEC_RUNTIME for every scenario at every NS                                 9
                                                                                                 = 37

MATRIX below has one row per case and names the instance it launches; _instance() restates the
dispatcher's rules in Python and test_matrix_reaches_every_rollout_kernel (CPU) holds the rows
against them.  The restatement is a copy, not a reading of the C++: whoever changes with_slots,
ActSpecs or launch_act changes _instance() / _reachable() in the same commit, and only then does a
new specialisation show up as a missing row.  The 37 counts the restated rules, not the kernels
the compiler emitted.

1. test_rollout_equals_single_ticks_matrix: one rollout launch of T ticks == T single acting ticks
   (swarm_act_step: the tick kernels, oracle-pinned by test_act_tick_parity*), bit for bit, with
   eps = 0.3, tick0 = 7, B = 38 (two dead waves in the last block), from the tie-heavy reset grid
   and from jittered half-spacing grids in contact.  Also pins what the launch's outputs are:
   reward the per-agent sum over the ticks, hits the per-env sum, avg_dist the LAST tick's mean goal
   distance, obs the final observation.
2. test_exploring_rollout_follows_the_oracle_closed_loop: the same launch against the oracle's own
   closed loop (graph -> forward -> eps-greedy -> env.step) with the Philox-keyed exploration on.
3. test_rollout_shard_keying: env_offset is in the coin's and the draw's key.
"""
import pytest
import torch

from oracle import swarm_oracle as O
from tests.conftest import assert_close_rel, record
from tests.test_gpu_parity import _rand_state, _tie_mask

gpu = pytest.mark.gpu

SCEN = {"GoTo": O.SCENARIO_GOTO, "ObstacleAvoidance": O.SCENARIO_OA, "Flocking": O.SCENARIO_FLOCK}
GRAPH = {"complete": O.GRAPH_COMPLETE, "knn": O.GRAPH_KNN, "radius": O.GRAPH_RADIUS}
T, T0, EPS, B1 = 6, 7, 0.3, 38
SCENS, NETS = ("GoTo", "ObstacleAvoidance", "Flocking"), ("gcn", "gat3")


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _instance(scen, N, graph, conv, net):
    """(NS, scenario, SPEC, net) of the act_kernel<NS, MODE_ROLLOUT, ...> a config launches:
    with_slots<8, 16, 32> and ActSpecs<NS, MODE_ROLLOUT, SCEN, NET>::allows, restated."""
    ns = 8 if N <= 8 else (16 if N <= 16 else 32)
    spec = "RUNTIME"
    if scen != "Flocking" and net == "gcn":
        if graph == "complete":
            spec = "COMPLETE_GAT" if conv == "gat" else "COMPLETE_GCN"
        elif graph == "knn" and conv == "gat":
            spec = "KNN_GAT"
        elif graph == "radius" and conv == "gat" and ns == 8 and scen == "GoTo":
            spec = "RADIUS_GAT"
    return ns, scen, spec, net


def _reachable():
    out = set()
    for scen in SCENS:
        for N in (8, 16, 32):
            for net in NETS:
                for graph in GRAPH:
                    for conv in (("gat", "gcn") if net == "gcn" else ("gat",)):   # GAT3 is GAT only (check_config)
                        out.add(_instance(scen, N, graph, conv, net))
    return out


# scenario, N, graph, k, conv, net -> act_kernel<NS, MODE_ROLLOUT, SCEN, SPEC, NET>
# (agent counts at the slot edges and inside: 1 2 5 8 | 9 12 16 | 17 20 29 32; k = N once, else 5 or 10)
G, OA, FL = "GoTo", "ObstacleAvoidance", "Flocking"
MATRIX = [
    # ---- 8 slots
    (G, 8, "complete", 0, "gat", "gcn"),      # < 8, GOTO, COMPLETE_GAT, GCN>
    (G, 5, "complete", 0, "gcn", "gcn"),      # < 8, GOTO, COMPLETE_GCN, GCN>
    (G, 8, "knn", 5, "gat", "gcn"),           # < 8, GOTO, KNN_GAT,      GCN>
    (G, 5, "radius", 0, "gat", "gcn"),        # < 8, GOTO, RADIUS_GAT,   GCN>
    (G, 5, "knn", 5, "gcn", "gcn"),           # < 8, GOTO, RUNTIME,      GCN>  kNN + GCNConv, k = N
    (G, 8, "radius", 0, "gcn", "gcn"),        # < 8, GOTO, RUNTIME,      GCN>  radius + GCNConv
    (G, 1, "complete", 0, "gat", "gcn"),      # < 8, GOTO, COMPLETE_GAT, GCN>  one agent
    (G, 1, "knn", 1, "gat", "gcn"),           # < 8, GOTO, KNN_GAT,      GCN>  one agent, k = 1
    (G, 2, "knn", 2, "gat", "gcn"),           # < 8, GOTO, KNN_GAT,      GCN>  two agents
    (OA, 5, "complete", 0, "gat", "gcn"),     # < 8, OA,   COMPLETE_GAT, GCN>
    (OA, 8, "complete", 0, "gcn", "gcn"),     # < 8, OA,   COMPLETE_GCN, GCN>
    (OA, 8, "knn", 5, "gat", "gcn"),          # < 8, OA,   KNN_GAT,      GCN>
    (OA, 8, "radius", 0, "gat", "gcn"),       # < 8, OA,   RUNTIME,      GCN>  radius + GAT
    (OA, 5, "radius", 0, "gcn", "gcn"),       # < 8, OA,   RUNTIME,      GCN>  radius + GCNConv
    (FL, 8, "complete", 0, "gat", "gcn"),     # < 8, FLOCK, RUNTIME,     GCN>
    (FL, 5, "knn", 5, "gat", "gcn"),          # < 8, FLOCK, RUNTIME,     GCN>
    (FL, 2, "complete", 0, "gat", "gcn"),     # < 8, FLOCK, RUNTIME,     GCN>  two agents
    (FL, 8, "knn", 5, "gat", "gat3"),         # < 8, FLOCK, RUNTIME,     GAT3>
    (G, 5, "complete", 0, "gat", "gat3"),     # < 8, GOTO, RUNTIME,      GAT3>
    (OA, 8, "radius", 0, "gat", "gat3"),      # < 8, OA,   RUNTIME,      GAT3>
    # ---- 16 slots
    (G, 12, "complete", 0, "gat", "gcn"),     # <16, GOTO, COMPLETE_GAT, GCN>
    (G, 9, "complete", 0, "gcn", "gcn"),      # <16, GOTO, COMPLETE_GCN, GCN>
    (G, 16, "knn", 10, "gat", "gcn"),         # <16, GOTO, KNN_GAT,      GCN>
    (G, 12, "radius", 0, "gat", "gcn"),       # <16, GOTO, RUNTIME,      GCN>  radius + GAT
    (G, 9, "knn", 5, "gcn", "gcn"),           # <16, GOTO, RUNTIME,      GCN>  kNN + GCNConv
    (OA, 16, "complete", 0, "gat", "gcn"),    # <16, OA,   COMPLETE_GAT, GCN>
    (OA, 12, "complete", 0, "gcn", "gcn"),    # <16, OA,   COMPLETE_GCN, GCN>
    (OA, 12, "knn", 10, "gat", "gcn"),        # <16, OA,   KNN_GAT,      GCN>
    (OA, 9, "radius", 0, "gat", "gcn"),       # <16, OA,   RUNTIME,      GCN>  radius + GAT
    (OA, 16, "radius", 0, "gcn", "gcn"),      # <16, OA,   RUNTIME,      GCN>  radius + GCNConv
    (FL, 9, "complete", 0, "gat", "gcn"),     # <16, FLOCK, RUNTIME,     GCN>
    (FL, 16, "knn", 5, "gat", "gcn"),         # <16, FLOCK, RUNTIME,     GCN>
    (FL, 12, "knn", 5, "gat", "gat3"),        # <16, FLOCK, RUNTIME,     GAT3>
    (G, 16, "radius", 0, "gat", "gat3"),      # <16, GOTO, RUNTIME,      GAT3>
    (OA, 9, "complete", 0, "gat", "gat3"),    # <16, OA,   RUNTIME,      GAT3>
    # ---- 32 slots: pair forces in place, the state in two register tiles, the 32-slot tie memo
    (G, 17, "complete", 0, "gat", "gcn"),     # <32, GOTO, COMPLETE_GAT, GCN>
    (G, 29, "complete", 0, "gcn", "gcn"),     # <32, GOTO, COMPLETE_GCN, GCN>
    (G, 32, "knn", 10, "gat", "gcn"),         # <32, GOTO, KNN_GAT,      GCN>
    (G, 20, "radius", 0, "gat", "gcn"),       # <32, GOTO, RUNTIME,      GCN>  radius + GAT
    (G, 17, "knn", 10, "gcn", "gcn"),         # <32, GOTO, RUNTIME,      GCN>  kNN + GCNConv
    (OA, 32, "complete", 0, "gat", "gcn"),    # <32, OA,   COMPLETE_GAT, GCN>
    (OA, 20, "complete", 0, "gcn", "gcn"),    # <32, OA,   COMPLETE_GCN, GCN>
    (OA, 29, "knn", 5, "gat", "gcn"),         # <32, OA,   KNN_GAT,      GCN>
    (OA, 17, "radius", 0, "gat", "gcn"),      # <32, OA,   RUNTIME,      GCN>  radius + GAT
    (OA, 29, "radius", 0, "gcn", "gcn"),      # <32, OA,   RUNTIME,      GCN>  radius + GCNConv
    (FL, 20, "complete", 0, "gat", "gcn"),    # <32, FLOCK, RUNTIME,     GCN>
    (FL, 29, "knn", 10, "gat", "gcn"),        # <32, FLOCK, RUNTIME,     GCN>
    (FL, 32, "knn", 5, "gat", "gat3"),        # <32, FLOCK, RUNTIME,     GAT3>
    (G, 17, "complete", 0, "gat", "gat3"),    # <32, GOTO, RUNTIME,      GAT3>
    (OA, 20, "knn", 10, "gat", "gat3"),       # <32, OA,   RUNTIME,      GAT3>
]


def _case_id(c):
    scen, N, graph, k, conv, net = c
    return f"{scen}-{N}-{graph}{k or ''}-{conv}-{net}"


def test_matrix_reaches_every_rollout_kernel():
    got = {_instance(scen, N, graph, conv, net) for scen, N, graph, k, conv, net in MATRIX}
    assert len(_reachable()) == 37
    assert got == _reachable(), sorted(_reachable() - got)
    # 17-32 agents: every scenario with both nets
    assert {(s, n) for ns, s, sp, n in got if ns == 32} == {(s, n) for s in SCENS for n in NETS}
    # the issue's rows: per NS and per GoTo / OA the four named graph / conv pairs and a runtime one
    for ns in (8, 16, 32):
        rows = [c for c in MATRIX if _instance(c[0], c[1], c[2], c[4], c[5])[0] == ns and c[5] == "gcn"]
        for scen in (G, OA):
            pairs = {(c[2], c[4]) for c in rows if c[0] == scen}
            assert {("complete", "gat"), ("complete", "gcn"), ("knn", "gat"), ("radius", "gat")} <= pairs
            assert pairs & {("knn", "gcn"), ("radius", "gcn")}
        assert {c[2] for c in rows if c[0] == FL} >= {"complete", "knn"}
    assert {c[1] for c in MATRIX} == {1, 2, 5, 8, 9, 12, 16, 17, 20, 29, 32}
    ks = [(c[1], c[3]) for c in MATRIX if c[2] == "knn"]
    assert any(k == n and n > 2 for n, k in ks) and all(k in (5, 10) or k == n for n, k in ks)


def _weights(golden_weights, scen, net, seed):
    if net == "gat3":
        return torch.tensor(golden_weights["flocking_gat3"][seed])
    # Flocking's one-layer net runs on GoTo's weights, as test_gpu_parity._params does
    return torch.tensor(golden_weights["obstacle_avoidance" if scen == OA else "go_to"][seed])


def _bits(a, b):
    """bit for bit (torch.equal would take -0.0 for +0.0)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _engine_pair(sw, golden_weights, case, B, seed=4, radius=0.3, **kw):
    scen, N, graph, k, conv, net = case
    p = _weights(golden_weights, scen, net, 3)
    args = dict(seed=seed, params=p, graph=graph, knn_k=max(k, 1), radius=radius, conv=conv, net=net, learn=False,
                eps=EPS, **kw)
    return sw.SwarmEngine(scen, N, B, **args), sw.SwarmEngine(scen, N, B, **args)


def _start_state(a, b, case, B):
    """envs [0, B/2): reset(0), the grid (kNN ties, radius pairs at the grid spacing and its
    multiples); envs [B/2, B): half-spacing grids with jitter, in contact from tick 0"""
    scen, N = case[0], case[1]
    a.reset(0)
    torch.cuda.synchronize()
    st = a.state.cpu()
    pos, vel = st[..., :2].clone(), st[..., 2:].clone()
    tp, tv = _rand_state(B - B // 2, N, 2 * N + 1, tight=True)
    pos[B // 2:], vel[B // 2:] = tp, tv
    for e in (a, b):
        e.set_state(pos, vel, fresh=True)
    if N > 1:   # some pair of the tight half starts within contact range
        f = O.pair_force(tp[:, :, None, :].expand(-1, N, N, 2), tp[:, None, :, :].expand(-1, N, N, 2))
        assert bool((f != 0).any())
    return pos, vel


def _single_ticks(b, n_ticks, tick0, eps):
    """n_ticks acting ticks of engine b; per tick its positions, mean goal distance and hits, and
    the rewards added up on the device in fp32, tick by tick (act_body's rew_sum order)"""
    rew = torch.zeros_like(b.reward)
    tp, td, th = [], [], []
    for t in range(n_ticks):
        b.ctrl[0] = tick0 + t
        b.set_eps(eps)
        b.act(push=False)
        rew += b.reward
        tp.append(b.state[..., :2].clone())
        td.append(b.avg_dist.clone())
        th.append(b.hits.clone())
    return rew, tp, td, th


def _assert_rollout_is_the_ticks(a, b, res, n_ticks, rew, tp, td, th, what):
    assert _bits(a.state, b.state), what
    if a.scenario_state is not None:
        assert _bits(a.scenario_state, b.scenario_state), what
    for t in range(n_ticks):
        assert _bits(res["traj_pos"][t], tp[t]), (what, t)
        assert _bits(res["traj_dist"][t], td[t]), (what, t)
        assert _bits(res["traj_hits"][t], th[t]), (what, t)
    assert _bits(res["hits"], res["traj_hits"].sum(0)), what         # small integers in fp32: exact in any order
    assert _bits(res["avg_dist"], res["traj_dist"][-1]), what        # the last tick's value, not a sum
    assert _bits(res["obs"][..., :4], a.state), what                 # the final observation
    assert torch.equal(res["obs"][..., 4:].cpu(), O.f32(O.GOAL).expand(a.B, a.N, 2)), what
    assert _bits(res["reward"], rew), what                           # per agent, summed in tick order


@gpu
@pytest.mark.parametrize("case", MATRIX, ids=_case_id)
def test_rollout_equals_single_ticks_matrix(sw, golden_weights, case):
    scen, N, graph, k, conv, net = case
    a, b = _engine_pair(sw, golden_weights, case, B1)
    _start_state(a, b, case, B1)
    res = a.rollout(T, tick0=T0, eps=EPS, traj=True)
    rew, tp, td, th = _single_ticks(b, T, T0, EPS)
    torch.cuda.synchronize()
    _assert_rollout_is_the_ticks(a, b, res, T, rew, tp, td, th, _case_id(case))
    # the exploration path ran: after the first tick, some env explores and some env does not
    coins = [O.egreedy(torch.zeros(B1, N, 9), EPS, 4, T0 + t)[1] for t in range(1, T)]
    assert any(bool(c.any()) and bool((~c).any()) for c in coins)
    assert sum(int(c.sum()) for c in coins) > 0


@gpu
def test_rollout_of_one_tick_is_one_acting_tick(sw, golden_weights):
    case = (OA, 12, "knn", 10, "gat", "gcn")
    a, b = _engine_pair(sw, golden_weights, case, B1)
    _start_state(a, b, case, B1)
    res = a.rollout(1, tick0=T0, eps=EPS, traj=True)
    rew, tp, td, th = _single_ticks(b, 1, T0, EPS)
    torch.cuda.synchronize()
    _assert_rollout_is_the_ticks(a, b, res, 1, rew, tp, td, th, "one tick")
    assert _bits(res["reward"], b.reward) and _bits(res["avg_dist"], b.avg_dist) and _bits(res["hits"], b.hits)
    assert _bits(res["obs"], b.obs)


@gpu
def test_rollout_of_no_ticks_touches_nothing(sw, golden_weights):
    from swarm_amd import _lib
    import ctypes
    case = (G, 20, "knn", 5, "gat", "gcn")
    N = case[1]
    a, b = _engine_pair(sw, golden_weights, case, B1)
    _start_state(a, b, case, B1)
    mark = 12345.0
    bufs = dict(reward=(B1, N), obs=(B1, N, 6), avg_dist=(B1,), hits=(B1,), traj_pos=(1, B1, N, 2), traj_dist=(1, B1),
                traj_hits=(1, B1))
    bufs = {n: torch.full(s, mark, device="cuda") for n, s in bufs.items()}
    out = _lib.SwarmActOut(0, 0, *[bufs[n].data_ptr() for n in ("reward", "obs", "avg_dist", "hits")], 0,
                           *[bufs[n].data_ptr() for n in ("traj_pos", "traj_dist", "traj_hits")])
    rc = a.lib.swarm_rollout(ctypes.byref(a.cfg), a.params.data_ptr(), a.state.data_ptr(), 0, T0, EPS, ctypes.byref(out),
                             _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert _bits(a.state, b.state)   # b never ran
    assert all(bool((v == mark).all()) for v in bufs.values())


# ------------------------------------------------------------------ 2. the oracle's closed loop, exploring
# scenario, N, graph, k, conv, B; the comment: envs the oracle itself keeps through all six ticks
LOOP_CASES = [
    (G, 8, "complete", 0, "gat", 64),      # 64/64
    (OA, 20, "knn", 10, "gat", 48),        # 44/48
    (OA, 29, "complete", 0, "gcn", 32),    # 32/32
    (FL, 12, "complete", 0, "gat", 48),    # 48/48
    (G, 16, "radius", 0, "gat", 48),       # 48/48
    (FL, 24, "knn", 6, "gat", 32),         # 32/32
    (G, 32, "knn", 10, "gat", 32),         # 32/32
]
L_SEED, L_T0, L_RADIUS = 21, 11, 0.3


def oracle_closed_loop(params, pos, vel, scen, graph, k, conv, n_ticks=T, eps=EPS, seed=L_SEED, tick0=L_T0,
                       radius=L_RADIUS):
    """O.act_tick fed its own output; per tick the step, the exploring envs and the envs still
    compared: an env leaves at its first tick where it did not explore (exploring ticks are
    Philox-keyed, hence exact) and some agent's top-2 Q gap is within 1e-4."""
    spread = O.flocking_reset_spread(pos) if scen == FL else None
    on = torch.ones(pos.shape[0], dtype=torch.bool)
    ticks = []
    for t in range(n_ticks):
        ref = O.act_tick(params, pos, vel, SCEN[scen], GRAPH[graph], k, eps, seed, tick0 + t, conv=conv,
                         radius=radius, prev_spread=spread)
        on = on & (ref.explore | _tie_mask(ref.q).all(-1))
        # the reset loop's stored spread is a magnitude of the first reward only; later ticks' is pos's own
        scale = O.flocking_reward_scale(pos, ref.step["pos"], spread if t == 0 else None) if scen == FL else None
        contact = ref.step["force"].ne(O.decode_actions(ref.actions)).any(-1)
        ticks.append(dict(step=ref.step, explore=ref.explore, on=on.clone(), scale=scale, contact=contact))
        pos, vel, spread = ref.step["pos"], ref.step["vel"], ref.step.get("spread")
    return ticks


@gpu
@pytest.mark.parametrize("scen,N,graph,k,conv,B", LOOP_CASES, ids=lambda v: str(v))
def test_exploring_rollout_follows_the_oracle_closed_loop(sw, golden_weights, scen, N, graph, k, conv, B):
    name = _case_id((scen, N, graph, k, conv, "gcn"))
    p = _weights(golden_weights, scen, "gcn", 3)
    eng = sw.SwarmEngine(scen, N, B, seed=L_SEED, params=p, graph=graph, knn_k=max(k, 1), radius=L_RADIUS, conv=conv,
                         learn=False, eps=EPS)
    eng.reset(0)
    torch.cuda.synchronize()
    pos, vel = eng.state.cpu()[..., :2].clone(), eng.state.cpu()[..., 2:].clone()
    r = eng.rollout(T, tick0=L_T0, eps=EPS, traj=True)
    torch.cuda.synchronize()
    tp, td, th = r["traj_pos"].cpu(), r["traj_dist"].cpu(), r["traj_hits"].cpu()
    ticks = oracle_closed_loop(O.unflatten_params(p), pos, vel, scen, graph, k, conv)
    worst = 0.0
    for t, tk in enumerate(ticks):
        on, step = tk["on"], tk["step"]
        e = (tp[t][on] - step["pos"][on]).abs().max().item() if on.any() else 0.0
        worst = max(worst, e)
        print(f"{name} tick {t}: {int(on.sum())}/{B} envs compared, {int(tk['explore'].sum())} exploring, "
              f"positions {e:.3e} from the oracle")
        assert e <= 1e-5, f"{name} tick {t}: rollout positions {e:.3e} from the oracle's closed loop"
        assert_close_rel(td[t][on], step["avg_dist"][on], 1e-6, f"{name} rollout tick {t} mean goal distance")
        assert torch.equal(th[t][on], step["hits"][on]), f"{name} tick {t}: hits"
    on = ticks[-1]["on"]
    n_on = int(on.sum())
    record(f"{name} exploring rollout vs oracle closed loop",
           {"max_abs": worst, "envs_compared_all_ticks": n_on, "of": B, "ticks": T,
            "exploring_per_tick": [int(tk["explore"].sum()) for tk in ticks],
            "agent_ticks_in_contact": sum(int(tk["contact"].sum()) for tk in ticks)})
    assert 4 * n_on >= 3 * B, f"{name}: too few envs outside the tie band to compare ({n_on}/{B})"
    assert any(bool(tk["explore"].any()) and bool((~tk["explore"]).any()) for tk in ticks[1:])
    assert sum(int(tk["contact"].sum()) for tk in ticks) > 0
    # the launch's outputs for the envs compared to the end
    want = sum(tk["step"]["rew"] for tk in ticks)
    if scen == FL:   # 2e-7 of the summed magnitudes the reward cancels (test_gpu_parity._assert_reward), per tick
        bound = sum(2e-7 * tk["scale"] for tk in ticks)[:, None].expand(B, N)
    else:            # 1e-6 relative (assert_close_rel's max(1, |r|)) per summed tick
        bound = sum(1e-6 * tk["step"]["rew"].double().abs().clamp_min(1.0) for tk in ticks)
    err = (r["reward"].cpu().double() - want.double()).abs()
    worst_r = (err / bound)[on].max().item()
    record(f"{name} exploring rollout summed reward", {"max_abs": err[on].max().item(), "max_err_over_bound": worst_r})
    print(f"{name}: summed reward error {err[on].max().item():.3e}, {worst_r:.3f} of its bound")
    assert worst_r <= 1.0, f"{name}: summed reward {worst_r:.2f}x its bound"
    assert torch.equal(r["hits"].cpu()[on], sum(tk["step"]["hits"] for tk in ticks)[on])
    assert_close_rel(r["avg_dist"].cpu()[on], ticks[-1]["step"]["avg_dist"][on], 1e-6, f"{name} last mean goal distance")


# ------------------------------------------------------------------ 3. shard keying
@gpu
def test_rollout_shard_keying(sw, golden_weights):
    """Envs 8..15 of a 16-env rollout == an 8-env rollout with env_offset = 8 from the same rows;
    envs 0..7 from those rows take other explored actions, so the offset is in the key."""
    N, tick0 = 8, 5
    kw = dict(seed=4, params=_weights(golden_weights, G, "gcn", 3), graph="knn", knn_k=5, learn=False, eps=EPS)
    full = sw.SwarmEngine(G, N, 16, **kw)
    shard = sw.SwarmEngine(G, N, 8, env_offset=8, **kw)
    plain = sw.SwarmEngine(G, N, 8, **kw)   # the same rows keyed as envs 0..7
    full.reset(0)
    torch.cuda.synchronize()
    st = full.state.cpu()
    for e in (shard, plain):
        e.set_state(st[8:, :, :2], st[8:, :, 2:])
    rf = full.rollout(T, tick0=tick0, eps=EPS, traj=True)
    rs = shard.rollout(T, tick0=tick0, eps=EPS, traj=True)
    rp = plain.rollout(T, tick0=tick0, eps=EPS, traj=True)
    torch.cuda.synchronize()
    assert _bits(shard.state, full.state[8:])
    assert _bits(rs["traj_pos"], rf["traj_pos"][:, 8:])
    assert _bits(rs["reward"], rf["reward"][8:]) and _bits(rs["avg_dist"], rf["avg_dist"][8:])
    # the keys differ where it matters: both key ranges explore somewhere, with other draws
    # (actions over an all-zero Q: 0 where the env is greedy, the random draw where it explores)
    lo = [O.egreedy(torch.zeros(8, N, 9), EPS, 4, tick0 + t, env_offset=0) for t in range(T)]
    hi = [O.egreedy(torch.zeros(8, N, 9), EPS, 4, tick0 + t, env_offset=8) for t in range(T)]
    assert any(bool(ex.any()) for _, ex, _ in lo) and any(bool(ex.any()) for _, ex, _ in hi)
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(lo, hi))
    assert not _bits(plain.state, shard.state)
    assert not _bits(rp["traj_pos"], rs["traj_pos"])
