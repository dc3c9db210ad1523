"""Population training on the GPU: member m of a SwarmPopulation computes bit for bit what a lone
SwarmEngine with that seed computes with train_tick.  Every comparison is torch.equal, and the
reference side is always lone engines, freshly built with the member's seed, never a population.
A case's lone runs are computed once and shared by the tests that need them."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS = (0, 4, 11)
COMMON = dict(eps=0.3, update_target_every=3)
# name -> (engine keyword arguments, ticks)
CASES = {
    # dead acting waves, a partial TD block, two 8-slot graphs per wave
    "goto5": (dict(scenario="GoTo", n_agents=5, n_envs=2, batch=3, replay_capacity=2 * 2), 8),
    # 16-slot kernels, a second acting block
    "oa12_gcn": (dict(scenario="ObstacleAvoidance", n_agents=12, n_envs=5, batch=5, replay_capacity=2 * 5,
                      conv="gcn"), 8),
    # one ring slot: every draw waits on a hand-off
    "goto8_radius": (dict(scenario="GoTo", n_agents=8, n_envs=4, batch=4, replay_capacity=1 * 4, graph="radius",
                          radius=0.3), 8),
    # the runtime kernel; stored scenario state
    "flocking6_knn": (dict(scenario="Flocking", n_agents=6, n_envs=3, batch=2, replay_capacity=3 * 3, graph="knn",
                           knn_k=5), 8),
    # the reference's own shape (default ring); updates start at tick 32
    "reference_shape": (dict(scenario="GoTo", n_agents=5, n_envs=1, batch=32), 40),
}
TICK_FIELDS = ("q", "actions", "reward", "samples", "grad", "ctrl")
FINAL_FIELDS = ("params", "adam_m", "adam_v", "target", "rep_s", "rep_s1", "rep_r", "rep_a", "_state_buf")


def _sw():
    import swarm_amd
    return swarm_amd


def _snap(eng):
    return {f: getattr(eng, f).clone() for f in TICK_FIELDS}


class LoneRun:
    """A lone engine ticked `ticks` times with train_tick: its per-tick snapshots, and the engine
    itself (left untouched afterwards) for the end-of-run comparison."""

    def __init__(self, kw, seed, ticks):
        sw = _sw()
        self.eng = eng = sw.SwarmEngine(seed=seed, **COMMON, **kw)
        eng.reset(0)
        self.snaps, self.slot_draws = [], 0
        for _ in range(ticks):
            eng.train_tick(full_out=True)
            self.snaps.append(_snap(eng))
        torch.cuda.synchronize()
        assert eng.handoff_errors() == 0
        # the ticks whose update ran, and the draws that came from the slot the tick was writing
        B, cap = eng.B, eng.capacity
        for t, s in enumerate(self.snaps):
            if int(s["ctrl"][7]):                     # trained: the batch of tick t was drawn
                slot = t % cap                        # write_slot of tick t
                self.slot_draws += int((s["samples"][: eng.batch] // B == slot).sum())
        self.adam_steps = int(self.snaps[-1]["ctrl"][3])


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


def run_population(case, seeds, ticks=None, check_every_tick=True):
    sw = _sw()
    kw, n = CASES[case]
    n = ticks or n
    refs = [lone(case, s, n) for s in seeds]
    # the inputs really exercise the learner and the hand-off (a guard on the case, not the kernel)
    assert all(r.adam_steps >= 1 for r in refs), [r.adam_steps for r in refs]
    assert sum(r.slot_draws for r in refs) >= 1
    pop = sw.SwarmPopulation(seeds=list(seeds), **COMMON, **kw)
    assert pop.P == len(seeds) and all(m.fused for m in pop.members)
    pop.reset(0)
    for t in range(n):
        pop.train_tick(full_out=True)
        if check_every_tick:
            for m, (s, r) in enumerate(zip(seeds, refs)):
                assert_tick_equal(pop.members[m], r.snaps[t], f"{case} seed {s} (member {m}) tick {t}")
    for m, (s, r) in enumerate(zip(seeds, refs)):
        assert_tick_equal(pop.members[m], r.snaps[n - 1], f"{case} seed {s} (member {m}) last tick")
        assert_final_equal(pop.members[m], r.eng, f"{case} seed {s} (member {m}) end")
    assert pop.handoff_errors() == [0] * len(seeds)
    pop.check_handoffs()
    assert [c["tick"] for c in pop.read_ctrl()] == [n] * len(seeds)
    return pop


@pytest.mark.parametrize("case", list(CASES))
def test_members_equal_lone_engines_bitwise(case):
    run_population(case, SEEDS)


def test_population_of_one_equals_the_lone_engine():
    run_population("goto5", (4,))


def test_member_order_does_not_matter():
    """(0, 4, 11) and (11, 0, 4): each seed gets the same bits wherever it sits (both orders are
    compared with the same lone runs)."""
    run_population("goto5", (0, 4, 11))
    run_population("goto5", (11, 0, 4))


def test_captured_episode_replays_as_eager_ticks():
    """A 6-tick episode captured once (one stream, no parallel branches) and replayed twice equals
    12 ticks of lone engines, and 12 eager population ticks."""
    sw = _sw()
    kw, _ = CASES["goto5"]
    refs = [lone("goto5", s, 12) for s in SEEDS]
    eager = run_population("goto5", SEEDS, ticks=12)
    pop = sw.SwarmPopulation(seeds=list(SEEDS), **COMMON, **kw)
    pop.reset(0)
    graph = pop.capture(6, lambda: pop.train_tick(full_out=True))
    # capture runs nothing: the members are still at tick 0
    assert [c["tick"] for c in pop.read_ctrl()] == [0, 0, 0]
    graph.replay()
    for m, r in enumerate(refs):
        assert_tick_equal(pop.members[m], r.snaps[5], f"member {m} after the first replay")
    graph.replay()
    torch.cuda.synchronize()
    for m, r in enumerate(refs):
        assert_tick_equal(pop.members[m], r.snaps[11], f"member {m} after the second replay")
        assert_final_equal(pop.members[m], r.eng, f"member {m} end (lone)")
        assert_final_equal(pop.members[m], eager.members[m], f"member {m} end (eager population)")
    assert pop.handoff_errors() == [0, 0, 0]


def test_more_blocks_than_the_chip_holds():
    """160 members x 6 blocks = 960 blocks against 768 resident (256 CUs x 3): the TD blocks of the
    late members start only as earlier blocks drain, and every hand-off still arrives (one ring
    slot: every draw waits on one), inside the fused tick's bounded waits."""
    sw = _sw()
    kw = dict(scenario="ObstacleAvoidance", n_agents=12, n_envs=8, batch=8, replay_capacity=8)
    P, ticks = 160, 3
    pop = sw.SwarmPopulation(seeds=list(range(P)), **COMMON, **kw)
    assert pop.members[0].capacity == 1
    pop.reset(0)
    for _ in range(ticks):
        pop.train_tick(full_out=True)
    torch.cuda.synchronize()
    assert pop.handoff_errors() == [0] * P
    for m in (0, 79, 159):
        ref = LoneRun(kw, m, ticks)
        assert ref.adam_steps >= 1 and ref.slot_draws >= 1
        assert_tick_equal(pop.members[m], ref.snaps[-1], f"member {m} last tick")
        assert_final_equal(pop.members[m], ref.eng, f"member {m} end")


def test_set_eps_scalar_and_per_member():
    sw = _sw()
    kw, _ = CASES["goto5"]
    pop = sw.SwarmPopulation(seeds=[0, 1, 2], **COMMON, **kw)
    pop.set_eps(0.5)
    assert [c["eps"] for c in pop.read_ctrl()] == [0.5] * 3
    pop.set_eps([0.25, 0.5, 0.75])
    assert [c["eps"] for c in pop.read_ctrl()] == [0.25, 0.5, 0.75]
    assert pop.members[2].read_ctrl()["eps"] == 0.75
    with pytest.raises(ValueError):
        pop.set_eps([0.1, 0.2])


def test_population_refuses_configurations_without_a_fused_tick():
    sw = _sw()
    with pytest.raises(ValueError):
        sw.SwarmPopulation(seeds=[0, 1], scenario="GoTo", n_agents=17, n_envs=2, batch=2, replay_capacity=4)
    a = sw.SwarmEngine("GoTo", 5, 2, seed=0, batch=2, replay_capacity=4)
    b = sw.SwarmEngine("GoTo", 5, 2, seed=1, batch=3, replay_capacity=4)
    with pytest.raises(ValueError):
        sw.SwarmPopulation.from_engines([a, b])   # two batch sizes


def _trainer(sw, seed, root):
    env = sw.make_env(scenario=sw.GoToPositionScenario(), num_envs=1, continuous_actions=False, wrapper=None,
                      max_steps=10, dict_spaces=True, n_agents=5, seed=seed)
    sw.set_seed(seed)
    return sw.DQNTrainer(env, seed, os.path.join(root, "models"), os.path.join(root, "stats"), "GoTo", batch_size=4,
                         replay_capacity=1000)


def test_population_trainer_equals_separate_trainers(tmp_path):
    sw = _sw()
    config = {"epsilon": 0.99, "epsilon_decay": 0.01, "min_epsilon": 0.05, "episodes": 3}
    seeds = (0, 1)
    lone_root, pop_root = str(tmp_path / "lone"), str(tmp_path / "pop")
    lone_tr = [_trainer(sw, s, lone_root) for s in seeds]
    for t in lone_tr:
        t.train_model(config)
    pop_tr = [_trainer(sw, s, pop_root) for s in seeds]
    sw.PopulationTrainer(pop_tr).train_model(config)
    for s, a, b in zip(seeds, lone_tr, pop_tr):
        assert a.engine.read_ctrl()["adam_step"] == b.engine.read_ctrl()["adam_step"] >= 1
        name = f"experiment_GoTo-seed_{s}"
        sa = torch.load(os.path.join(lone_root, "models", name + ".pth"))
        sb = torch.load(os.path.join(pop_root, "models", name + ".pth"))
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"seed {s}: {k}"
        ca = open(os.path.join(lone_root, "stats", name + ".csv"), "rb").read()
        cb = open(os.path.join(pop_root, "stats", name + ".csv"), "rb").read()
        assert ca == cb and ca.startswith(b"Episode,Reward,Loss")
        # 3 episodes write no CSV row (the reference writes one per 10): the lists behind it too
        assert a.episode_losses == b.episode_losses and len(a.episode_losses) == 3
        assert [float(x) for x in a.rewards_buffer] == [float(x) for x in b.rewards_buffer]
        assert a.writer.scalars["Loss"] == b.writer.scalars["Loss"] and len(a.writer.scalars["Loss"]) >= 1
        # 'Reward' is torch's sum of the 5 agents' rewards, over [B, N] there and [P, B, N] here:
        # torch does not pin a reduction's order across shapes, so this one value is compared to
        # the rounding of a 5-term fp32 sum of one sign, 2 * 4 * 2^-24 < 1e-6 relative
        ra, rb = a.writer.scalars["Reward"], b.writer.scalars["Reward"]
        assert [s for s, _ in ra] == [s for s, _ in rb] == list(range(1, 31))
        assert all(abs(x - y) <= 1e-6 * abs(x) for (_, x), (_, y) in zip(ra, rb))
