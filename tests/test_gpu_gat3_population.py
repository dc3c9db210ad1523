"""Populations of three-layer GAT learners on the GPU: member m of a SwarmGat3Population computes bit
for bit what a lone SwarmGat3Engine with that seed computes with train_tick.  Every comparison is
torch.equal, and the reference side is always lone engines, freshly built with the member's seed and
hyper-parameters, never a population.  A case's lone runs are computed once and shared by the tests
that need them."""
import contextlib
import io
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS = (0, 4, 11)
COMMON = dict(eps=0.3, update_target_every=3)
# name -> (engine keyword arguments, ticks)
CASES = {
    # 8-slot kernels; ticks 0-2 skip (2, 4, 6 graphs < 7), tick 3 on trains, the 4-slot ring wraps; the
    # second TD block has three live waves and one idle one
    "n5_complete": (dict(scenario="Flocking", n_agents=5, n_envs=2, batch=7, replay_capacity=8), 10),
    # 16-slot kernels, a second acting block with dead waves
    "n12_knn": (dict(scenario="Flocking", n_agents=12, n_envs=5, batch=5, graph="knn", knn_k=5, replay_capacity=10), 8),
    # 32-slot kernels, two waves per block
    "n17_radius": (dict(scenario="Flocking", n_agents=17, n_envs=2, batch=3, graph="radius", radius=0.5,
                        replay_capacity=4), 6),
    # the reference's own shape (default ring); updates start at tick 31
    "reference_shape": (dict(scenario="Flocking", n_agents=10, n_envs=1, batch=32), 36),
    # another scenario's acting kernel (SwarmGat3Engine runs every scenario)
    "oa8": (dict(scenario="ObstacleAvoidance", n_agents=8, n_envs=3, batch=4, replay_capacity=9), 6),
}
TICK_FIELDS = ("q", "actions", "reward", "samples", "grad", "ctrl")
FINAL_FIELDS = ("params", "adam_m", "adam_v", "target", "rep_s", "rep_s1", "rep_r", "rep_a", "_state_buf")
ADAM_STEP = 3   # word of ctrl


def _sw():
    import swarm_amd
    return swarm_amd


def _snap(eng):
    return {f: getattr(eng, f).clone() for f in TICK_FIELDS}


class LoneRun:
    """A lone SwarmGat3Engine ticked `ticks` times with train_tick: its per-tick snapshots, and the
    engine itself (left untouched afterwards) for the end-of-run comparison.  ``events``: {tick t:
    fn(engine)} called in front of tick t."""

    def __init__(self, kw, seed, ticks, events=None):
        self.eng = eng = _sw().SwarmGat3Engine(seed=seed, **{**COMMON, **kw})
        eng.reset(0)
        self.snaps = []
        for t in range(ticks):
            if events and t in events:
                events[t](eng)
            eng.train_tick(full_out=True)
            self.snaps.append(_snap(eng))
        torch.cuda.synchronize()
        steps = [0] + [int(s["ctrl"][ADAM_STEP]) for s in self.snaps]
        self.adam_steps = steps[-1]
        self.skipped = sum(1 for a, b in zip(steps, steps[1:]) if a == b)


_LONE = {}


def lone(case, seed, ticks=None):
    kw, n = CASES[case]
    n = ticks or n
    key = (case, seed, n)
    if key not in _LONE:
        _LONE[key] = LoneRun(kw, seed, n)
    return _LONE[key]


def assert_tick_equal(member, ref_snap, what):
    for f in TICK_FIELDS:
        assert torch.equal(getattr(member, f), ref_snap[f]), f"{what}: {f}"


def assert_final_equal(member, ref_eng, what):
    for f in FINAL_FIELDS:
        assert torch.equal(getattr(member, f), getattr(ref_eng, f)), f"{what}: {f}"
    if ref_eng.scenario_state is not None:   # Flocking's stored spread (inside _state_buf; named for the message)
        assert torch.equal(member.scenario_state, ref_eng.scenario_state), f"{what}: scenario_state"


def check_guards(case, refs):
    """the inputs really exercise the learner and the skip rule (a guard on the case, not the kernel)"""
    assert all(r.adam_steps >= 1 for r in refs), [r.adam_steps for r in refs]
    if case == "n5_complete":
        assert all(r.skipped >= 1 for r in refs), [r.skipped for r in refs]


def tick_and_compare(pop, refs, n, what, events=None):
    for t in range(n):
        if events and t in events:
            events[t](pop)
        pop.train_tick(full_out=True)
        for m, r in enumerate(refs):
            assert_tick_equal(pop.members[m], r.snaps[t], f"{what} member {m} tick {t}")
    for m, r in enumerate(refs):
        assert_final_equal(pop.members[m], r.eng, f"{what} member {m} end")
    assert [c["tick"] for c in pop.read_ctrl()] == [n] * pop.P


def run_population(case, seeds, ticks=None):
    sw = _sw()
    kw, n = CASES[case]
    n = ticks or n
    refs = [lone(case, s, n) for s in seeds]
    check_guards(case, refs)
    pop = sw.SwarmGat3Population(seeds=list(seeds), **COMMON, **kw)
    assert pop.P == len(seeds) and all(type(m) is sw.SwarmGat3Engine for m in pop.members)
    assert not pop.per_member_hp
    pop.reset(0)
    tick_and_compare(pop, refs, n, f"{case} seeds {seeds}")
    pop.flush()   # nothing pending: nothing moves
    for m, r in enumerate(refs):
        assert_final_equal(pop.members[m], r.eng, f"{case} member {m} after flush")
    return pop


# ------------------------------------------------------------------ 1. member equals lone
@pytest.mark.parametrize("case", list(CASES))
def test_members_equal_lone_engines_bitwise(case):
    run_population(case, SEEDS)


# ------------------------------------------------------------------ 2. independence
def test_population_of_one_equals_the_lone_engine():
    run_population("n5_complete", (4,))


def test_member_order_and_company_do_not_matter():
    """seed 0 gets the same bits in (0, 4, 11) and in (11, 0) (both compared with the same lone run)"""
    run_population("n5_complete", (0, 4, 11))
    run_population("n5_complete", (11, 0))


def test_two_members_with_one_seed_are_bitwise_equal():
    pop = run_population("n5_complete", (4, 4))
    a, b = pop.members
    for f in TICK_FIELDS + FINAL_FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.params.data_ptr() != b.params.data_ptr() and a.rep_s.data_ptr() != b.rep_s.data_ptr()


# ------------------------------------------------------------------ 3. per-member hyper-parameters
SWEEP = dict(lr=[1e-3, 3e-3, 5e-4], gamma=[0.99, 0.9, 0.95], betas=[(0.9, 0.999), (0.8, 0.99), (0.85, 0.995)],
             adam_eps=[1e-8, 1e-6, 1e-7], max_norm=[1.0, 0.05, 10.0], update_target_every=[3, 2, 4])
CHANGE_AT = 6   # set_member_hp / set_hp in front of this tick: updates ran before it and run after it
CHANGE = dict(lr=2e-3, gamma=0.8, betas=(0.7, 0.9), adam_eps=1e-5, max_norm=0.01, update_target_every=2)


def test_per_member_hyper_parameters_and_set_member_hp():
    sw = _sw()
    kw, n = CASES["n5_complete"]
    change = {CHANGE_AT: lambda eng: eng.set_hp(**CHANGE)}
    refs = [LoneRun({**kw, **{k: v[m] for k, v in SWEEP.items()}}, s, n, change if m == 1 else None)
            for m, s in enumerate(SEEDS)]
    check_guards("n5_complete", refs)
    assert refs[1].snaps[CHANGE_AT - 1]["ctrl"][ADAM_STEP] >= 1   # the change has a transition step
    pop = sw.SwarmGat3Population(seeds=list(SEEDS), **{**COMMON, **kw, **SWEEP})
    assert pop.per_member_hp
    pop.reset(0)
    tick_and_compare(pop, refs, n, "sweep", {CHANGE_AT: lambda p: p.set_member_hp(1, **CHANGE)})
    # the members differ where their rows do
    assert not torch.equal(pop.members[0].params, pop.members[1].params)
    with pytest.raises(ValueError):
        pop.set_member_hp(3, lr=1e-3)
    with pytest.raises(ValueError):
        pop.set_member_hp(0, update_target_every=0)
    with pytest.raises(ValueError):
        sw.SwarmGat3Population(seeds=[0, 1], **{**COMMON, **kw, "lr": [1e-3, 1e-3, 1e-3]})


def test_equal_rows_run_the_shared_path_with_the_table_paths_bits():
    sw = _sw()
    kw, n = CASES["n5_complete"]
    refs = [lone("n5_complete", s) for s in SEEDS]
    one = {k: [v[0]] * 3 for k, v in SWEEP.items()}   # sequences, all rows equal (COMMON's values)
    pop = sw.SwarmGat3Population(seeds=list(SEEDS), **{**COMMON, **kw, **one})
    assert not pop.per_member_hp
    pop.per_member_hp = True   # the same rows through the table
    pop.reset(0)
    tick_and_compare(pop, refs, n, "equal rows, table path")
    shared = run_population("n5_complete", SEEDS)   # and as kernel arguments
    for a, b in zip(pop.members, shared.members):
        assert_final_equal(a, b, "table path against shared path")


# ------------------------------------------------------------------ 4. capture
def test_captured_ticks_replay_as_eager_ticks_and_see_new_rows_and_eps():
    """A 5-tick graph replayed twice, the optimizer row of member 1 and every member's eps rewritten
    between the replays: 10 eager ticks of lone engines with the same change in front of tick 5."""
    sw = _sw()
    kw, _ = CASES["n5_complete"]
    eps2 = [0.1, 0.6, 0.9]
    new = dict(lr=4e-3, gamma=0.7, update_target_every=1)

    def lone_events(m):
        def at5(eng):
            eng.set_eps(eps2[m])
            if m == 1:
                eng.set_hp(**new)
        return {5: at5}
    refs = [LoneRun(kw, s, 10, lone_events(m)) for m, s in enumerate(SEEDS)]
    check_guards("n5_complete", refs)
    pop = sw.SwarmGat3Population(seeds=list(SEEDS), **COMMON, **kw)
    pop.per_member_hp = True   # before the capture: a row will change
    pop.reset(0)
    graph = pop.capture(5, lambda: pop.train_tick(full_out=True))
    assert [c["tick"] for c in pop.read_ctrl()] == [0, 0, 0]   # capture runs nothing
    graph.replay()
    for m, r in enumerate(refs):
        assert_tick_equal(pop.members[m], r.snaps[4], f"member {m} after the first replay")
    pop.set_member_hp(1, **new)
    pop.set_eps(eps2)
    graph.replay()
    torch.cuda.synchronize()
    for m, r in enumerate(refs):
        assert_tick_equal(pop.members[m], r.snaps[9], f"member {m} after the second replay")
        assert_final_equal(pop.members[m], r.eng, f"member {m} end")
    # the change did something: member 1 without it ends elsewhere
    assert not torch.equal(refs[1].eng.params, lone("n5_complete", SEEDS[1]).eng.params)


# ------------------------------------------------------------------ 5. evaluate
def test_evaluate_equals_lone_rollouts_and_leaves_training_alone():
    sw = _sw()
    from swarm_amd.population import evaluation_engine
    kw, n = CASES["n12_knn"]
    refs = [lone("n12_knn", s) for s in SEEDS]
    check_guards("n12_knn", refs)
    pop = sw.SwarmGat3Population(seeds=list(SEEDS), **COMMON, **kw)
    pop.reset(0)
    half = n // 2
    for _ in range(half):
        pop.train_tick(full_out=True)
    assert all(c["adam_step"] >= 1 for c in pop.read_ctrl())   # trained weights are evaluated
    res = {k: v.clone() for k, v in pop.evaluate(3, 5, seed=99, episode=2).items()}
    for m, e in enumerate(pop.members):
        ev = evaluation_engine(e.cfg, 3, 99)
        ev.reset(2)
        want = ev.rollout(5, tick0=0, eps=0.0, params=e.params)
        for k in want:
            assert torch.equal(res[k][m], want[k]), f"member {m}: {k}"
    assert not torch.equal(res["reward"][0], res["reward"][1])   # two policies, one set of envs
    for t in range(half, n):
        pop.train_tick(full_out=True)
        for m, r in enumerate(refs):
            assert_tick_equal(pop.members[m], r.snaps[t], f"member {m} tick {t} after the evaluation")
    for m, r in enumerate(refs):
        assert_final_equal(pop.members[m], r.eng, f"member {m} end")


# ------------------------------------------------------------------ 6. the trainer
def _trainer(sw, seed, root, net="gat3", **kw):
    env = sw.make_env(scenario=sw.FlockingScenario(), num_envs=4, continuous_actions=False, wrapper=None, max_steps=6,
                      dict_spaces=True, n_agents=4, seed=seed)
    sw.set_seed(seed)
    return sw.DQNTrainer(env, seed, os.path.join(root, "models"), os.path.join(root, "stats"), "Flocking", net=net,
                         batch_size=8, replay_capacity=1000, **kw)


def test_population_trainer_equals_separate_trainers(tmp_path):
    sw = _sw()
    config = {"epsilon": 0.99, "epsilon_decay": 0.01, "min_epsilon": 0.05, "episodes": 2, "eval_every": 1,
              "eval_envs": 3}
    seeds = (1, 2)
    lone_root, pop_root = str(tmp_path / "lone"), str(tmp_path / "pop")
    with contextlib.redirect_stdout(io.StringIO()):
        lone_tr = [_trainer(sw, s, lone_root) for s in seeds]
        for t in lone_tr:
            t.train_model(config)
        pop_tr = [_trainer(sw, s, pop_root) for s in seeds]
        driver = sw.Gat3PopulationTrainer(pop_tr)
        assert isinstance(driver.population, sw.SwarmGat3Population)
        with pytest.raises(ValueError, match="pbt_every"):
            driver.train_model(dict(config, pbt_every=1))
        driver.train_model(config)   # the second episode is captured and replayed
    for s, a, b in zip(seeds, lone_tr, pop_tr):
        assert a.engine.read_ctrl()["adam_step"] == b.engine.read_ctrl()["adam_step"] == 11
        name = f"experiment_Flocking-seed_{s}"
        sa = torch.load(os.path.join(lone_root, "models", name + ".pth"), weights_only=True)
        sb = torch.load(os.path.join(pop_root, "models", name + ".pth"), weights_only=True)
        assert list(sa) == list(sb) and len(sa) == 16
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"seed {s}: {k}"
        for sfx, head in ((".csv", b"Episode,Reward,Loss"), ("-eval.csv", b"Episode,Reward,Collisions,Distance (end)")):
            ca = open(os.path.join(lone_root, "stats", name + sfx), "rb").read()
            cb = open(os.path.join(pop_root, "stats", name + sfx), "rb").read()
            assert ca == cb and ca.startswith(head), sfx
        assert a.eval_rows == b.eval_rows and len(a.eval_rows) == 2
        assert a.episode_losses == b.episode_losses and len(a.episode_losses) == 2
        assert [float(x) for x in a.rewards_buffer] == [float(x) for x in b.rewards_buffer]
        # 'Loss' is logged by the ticks whose adam_step advanced: every tick but the first (4 graphs < 8)
        assert [t for t, _ in a.writer.scalars["Loss"]] == list(range(2, 13))
        print("Reward scalars, lone and population:", a.writer.scalars["Reward"], b.writer.scalars["Reward"])
        assert a.writer.scalars == b.writer.scalars
    assert pop_tr[0].eval_rows != pop_tr[1].eval_rows


def test_population_trainer_with_differing_trainers_and_epsilons(tmp_path):
    """lr, gamma, update_target_every per trainer and the epsilon schedule per member: each member is
    its lone trainer (that trainer's values, its own scalar schedule)"""
    sw = _sw()
    hp = (dict(lr=1e-3, gamma=0.99, update_target_every=200), dict(lr=3e-3, gamma=0.9, update_target_every=2))
    eps = ([0.99, 0.5], [0.01, 0.3], [0.05, 0.1])
    config = {"epsilon": eps[0], "epsilon_decay": eps[1], "min_epsilon": eps[2], "episodes": 2}
    seeds = (1, 2)
    with contextlib.redirect_stdout(io.StringIO()):
        pop_tr = [_trainer(sw, s, str(tmp_path / "pop"), **hp[m]) for m, s in enumerate(seeds)]
        driver = sw.Gat3PopulationTrainer(pop_tr)
        assert driver.population.per_member_hp
        driver.train_model(config)
        for m, s in enumerate(seeds):
            t = _trainer(sw, s, str(tmp_path / "lone"), **hp[m])
            t.train_model(dict(config, epsilon=eps[0][m], epsilon_decay=eps[1][m], min_epsilon=eps[2][m]))
            assert t.engine.read_ctrl()["adam_step"] == 11
            for k in ("_lrn", "grad", "rep_s", "rep_s1", "rep_r", "rep_a", "_state_buf", "ctrl", "samples"):
                assert torch.equal(getattr(t.engine, k), getattr(pop_tr[m].engine, k)), f"trainer {m}: {k}"
            assert t.writer.scalars["Loss"] == pop_tr[m].writer.scalars["Loss"]


# ------------------------------------------------------------------ 7. refusals
def test_refusals(tmp_path):
    sw = _sw()
    kw = dict(n_agents=5, n_envs=2, batch=3, replay_capacity=4)
    g = [sw.SwarmGat3Engine("Flocking", seed=s, **kw) for s in (0, 1)]
    one_layer = sw.SwarmEngine("Flocking", seed=2, **kw)
    acting = sw.SwarmEngine("Flocking", seed=2, net="gat3", learn=False, params=g[0].params.clone(), **kw)
    pop_of = sw.SwarmGat3Population.from_engines
    for bad, why in ((one_layer, "SwarmGat3Engine"), (acting, "SwarmGat3Engine")):
        with pytest.raises(ValueError, match=why):
            pop_of([g[0], bad])
    for other in (dict(kw, n_agents=6), dict(kw, graph="knn", knn_k=3), dict(kw, batch=2), dict(kw, replay_capacity=8),
                  dict(kw, scenario="GoTo")):
        args = dict(dict(scenario="Flocking"), **other)
        with pytest.raises(ValueError, match="share"):
            pop_of([g[0], sw.SwarmGat3Engine(seed=1, **args)])
    with pytest.raises(ValueError, match="once"):
        pop_of([g[0], g[1], g[0]])
    with pytest.raises(ValueError):
        pop_of([])
    with pytest.raises(ValueError):
        sw.SwarmGat3Population(seeds=[0, 1], seed=3, scenario="Flocking", **kw)
    # the one-layer network's population and trainer stay closed to these learners
    with pytest.raises(ValueError, match="SwarmGat3Population"):
        sw.SwarmPopulation.from_engines(g)
    with pytest.raises(ValueError):
        sw.SwarmEngine("Flocking", net="gat3", learn=True, **kw)
    pop = pop_of(g)
    score = torch.zeros(2, device=pop.device)
    with pytest.raises(ValueError, match="swarm_pop_member"):
        pop.exploit(score, round=0)
    for fn in (pop.handoff_errors, pop.check_handoffs):
        with pytest.raises(ValueError, match="hand-off"):
            fn()
    with pytest.raises(ValueError):
        pop.set_eps([0.1, 0.2, 0.3])
    pop.reset(0)
    pop.train_tick()   # the refusals left a population that ticks
    assert [c["tick"] for c in pop.read_ctrl()] == [1, 1]
    gat3_tr = _trainer(sw, 1, str(tmp_path))
    gcn_tr = _trainer(sw, 1, str(tmp_path), net="gcn")
    with pytest.raises(ValueError, match="Gat3PopulationTrainer"):
        sw.PopulationTrainer([gat3_tr])
    with pytest.raises(ValueError, match="PopulationTrainer"):
        sw.Gat3PopulationTrainer([gat3_tr, gcn_tr])
