"""Per-member optimizer hyper-parameters on the GPU: member m of a SwarmPopulation whose members
differ in lr, gamma, betas, adam_eps, max_norm and update_target_every computes bit for bit what a
lone SwarmEngine built with member m's values computes with train_tick.  The method is
tests/test_gpu_population.py's: every comparison is torch.equal, of that file's TICK_FIELDS after
every tick and its FINAL_FIELDS at the end; the reference side is always freshly built lone
engines, never a population; hand-off error words are 0.  A lone run is computed once and shared
by the tests that need it."""
import os

import pytest
import torch

from tests.test_gpu_population import CASES, SEEDS, _snap, assert_final_equal, assert_tick_equal

pytestmark = pytest.mark.gpu

EPS = 0.3
# member 0 of the one-field test: the engine's defaults with update_target_every = 3
DEFAULT = dict(lr=1e-3, gamma=0.99, betas=(0.9, 0.999), adam_eps=1e-8, max_norm=1.0, update_target_every=3)
# one field at a time against DEFAULT.  betas[0] only shows from the second optimizer step on (the
# first step's m / (1 - beta1) is the gradient whatever beta1 is): the guards ask for two steps.
ONE_FIELD = (
    dict(lr=3e-3),
    dict(gamma=0.5),
    dict(betas=(0.5, 0.999)),
    dict(betas=(0.9, 0.9)),
    dict(adam_eps=1e-3),
    dict(max_norm=1e-3),             # far below the gradient norm (asserted): the clip bites
    dict(update_target_every=2),
)
# three members, every field distinct; max_norm: never clips / always clips (both asserted) / in between
BIG_NORM, SMALL_NORM = 1e6, 1e-4
MEMBERS = (
    (0, dict(lr=1e-3, gamma=0.99, betas=(0.9, 0.999), adam_eps=1e-8, max_norm=BIG_NORM, update_target_every=2)),
    (4, dict(lr=3e-3, gamma=0.9, betas=(0.8, 0.99), adam_eps=1e-5, max_norm=SMALL_NORM, update_target_every=3)),
    (11, dict(lr=3e-4, gamma=0.5, betas=(0.5, 0.9), adam_eps=1e-3, max_norm=0.05, update_target_every=5)),
)


def _sw():
    import swarm_amd
    return swarm_amd


def _freeze(d):
    return tuple(sorted(d.items()))


class Lone:
    """A lone engine built with `hp`, ticked `ticks` times with train_tick(full_out=True): its
    per-tick snapshots and the engine itself, left untouched afterwards.  change = (t, fields):
    set_hp(**fields) after t ticks."""

    def __init__(self, case, seed, hp, ticks, change=None):
        kw, _ = CASES[case]
        self.eng = eng = _sw().SwarmEngine(seed=seed, eps=EPS, **hp, **kw)
        eng.reset(0)
        self.snaps = []
        for t in range(ticks):
            if change is not None and t == change[0]:
                eng.set_hp(**change[1])
            eng.train_tick(full_out=True)
            self.snaps.append(_snap(eng))
        torch.cuda.synchronize()
        assert eng.handoff_errors() == 0
        self.adam_steps = int(self.snaps[-1]["ctrl"][3])
        # the pre-clip gradient norms the optimizer steps saw (word 6; 0 until the first step ran)
        norms = [float(s["ctrl"].view(torch.float32)[6]) for s in self.snaps]
        self.grad_norms = [g for g in norms if g != 0.0]


_LONE = {}


def lone(case, seed, hp, ticks=8, change=None):
    key = (case, seed, _freeze(hp), ticks, change and (change[0], _freeze(change[1])))
    if key not in _LONE:
        _LONE[key] = Lone(case, seed, hp, ticks, change)
    return _LONE[key]


def columns(hps):
    """[{field: value}] per member -> {field: [value per member]}: SwarmPopulation's keyword arguments"""
    return {k: [hp[k] for hp in hps] for k in hps[0]}


def run_population(case, members, refs, ticks=8, force_hp=None, expect_hp=True):
    """members: [(seed, hp)]; refs: their lone runs.  Every tick and the end, bit for bit."""
    sw = _sw()
    kw, _ = CASES[case]
    pop = sw.SwarmPopulation(seeds=[s for s, _ in members], eps=EPS, **columns([hp for _, hp in members]), **kw)
    assert pop.P == len(members) and all(e.fused for e in pop.members)
    assert pop.per_member_hp is expect_hp
    if force_hp is not None:
        pop.per_member_hp = force_hp
    pop.reset(0)
    for t in range(ticks):
        pop.train_tick(full_out=True)
        for m, r in enumerate(refs):
            assert_tick_equal(pop.members[m], r.snaps[t], f"{case} member {m} tick {t}")
    for m, r in enumerate(refs):
        assert_final_equal(pop.members[m], r.eng, f"{case} member {m} end")
    assert pop.handoff_errors() == [0] * len(members)
    pop.check_handoffs()
    assert [c["tick"] for c in pop.read_ctrl()] == [ticks] * len(members)
    return pop


def test_one_field_at_a_time_one_seed():
    """Eight members with ONE seed: the defaults, and seven that differ from them in exactly one
    field.  The guards show that each field changes a lone run's weights, so a member that read
    another member's (or the shared) value for it could not equal its lone run."""
    hps = [dict(DEFAULT)] + [dict(DEFAULT, **f) for f in ONE_FIELD]
    refs = [lone("goto5", 4, hp) for hp in hps]
    base = refs[0]
    for hp, r in zip(hps, refs):
        assert r.adam_steps >= 2, (hp, r.adam_steps)
    for f, r in zip(ONE_FIELD, refs[1:]):
        assert not (torch.equal(r.eng.params, base.eng.params) and torch.equal(r.eng.target, base.eng.target)), f
    # the small max_norm really clips: every step's gradient norm is far above it
    assert len(base.grad_norms) >= 2 and min(refs[6].grad_norms) > 10 * ONE_FIELD[5]["max_norm"], refs[6].grad_norms
    run_population("goto5", [(4, hp) for hp in hps], refs)


def _member_refs(case, members=MEMBERS):
    refs = [lone(case, s, hp) for s, hp in members]
    assert all(r.adam_steps >= 2 for r in refs), [r.adam_steps for r in refs]
    by_norm = {hp["max_norm"]: r for (_, hp), r in zip(members, refs)}
    big, small = by_norm[BIG_NORM].grad_norms, by_norm[SMALL_NORM].grad_norms
    assert len(big) >= 2 and max(big) < BIG_NORM, big        # the clip never bites
    assert len(small) >= 2 and min(small) > SMALL_NORM, small   # the clip always bites
    return refs


@pytest.mark.parametrize("case", ["oa12_gcn", "goto8_radius", "flocking6_knn"])
def test_everything_different_at_once(case):
    """Distinct seeds and all seven fields distinct, on the 16-slot kernels, with a one-slot ring
    (every draw waits on a hand-off) and on the runtime kernel; target syncs every 2, 3 and 5 ticks."""
    run_population(case, list(MEMBERS), _member_refs(case))


def test_member_order_does_not_matter():
    refs = _member_refs("oa12_gcn")
    order = (2, 0, 1)
    run_population("oa12_gcn", [MEMBERS[i] for i in order], [refs[i] for i in order])


def test_uniform_rows_take_the_shared_entry_points():
    """Sequences whose values are all equal: the population reports per_member_hp False and ticks
    with swarm_pop_train_tick / swarm_pop_reduce_advance as before; forced onto the _hp pair, the
    equal rows give the same bits."""
    members = [(s, dict(DEFAULT)) for s in SEEDS]
    refs = [lone("goto5", s, hp) for s, hp in members]
    assert all(r.adam_steps >= 2 for r in refs)
    pop = run_population("goto5", members, refs, expect_hp=False)
    assert pop.per_member_hp is False
    pop = run_population("goto5", members, refs, expect_hp=False, force_hp=True)
    assert pop.per_member_hp is True


def test_captured_episode_sees_a_rewritten_row():
    """A 6-tick episode captured once (one stream) and replayed twice equals 12 lone ticks.  Then
    member 1's lr and gamma change (set_member_hp) and the SAME graph is replayed once more: member
    1 equals a lone engine whose hp changed after its 12th eager tick, the others their unchanged
    lone runs.  The rows are read from device memory on every launch; a kernel-argument hp would
    be frozen into the graph."""
    sw = _sw()
    kw, _ = CASES["goto5"]
    members = [(s, dict(DEFAULT, **f)) for s, f in zip(SEEDS, (dict(lr=1e-3), dict(lr=3e-3, gamma=0.9),
                                                               dict(update_target_every=2)))]
    new = dict(lr=2e-4, gamma=0.6)
    refs = [lone("goto5", s, hp, ticks=18, change=(12, new) if m == 1 else None) for m, (s, hp) in enumerate(members)]
    # the change matters: member 1's unchanged lone run ends elsewhere
    same = lone("goto5", members[1][0], members[1][1], ticks=18)
    assert not torch.equal(same.eng.params, refs[1].eng.params)
    assert all(torch.equal(a["grad"], b["grad"]) for a, b in zip(same.snaps[:12], refs[1].snaps[:12]))
    pop = sw.SwarmPopulation(seeds=[s for s, _ in members], eps=EPS, **columns([hp for _, hp in members]), **kw)
    assert pop.per_member_hp is True
    pop.reset(0)
    graph = pop.capture(6, lambda: pop.train_tick(full_out=True))
    assert [c["tick"] for c in pop.read_ctrl()] == [0, 0, 0]   # capture runs nothing
    for upto in (5, 11):
        graph.replay()
        for m, r in enumerate(refs):
            assert_tick_equal(pop.members[m], r.snaps[upto], f"member {m} after tick {upto + 1}")
    pop.set_member_hp(1, **new)
    assert pop.members[1].hp.lr_d == new["lr"] and abs(pop.members[1].hp.gamma - new["gamma"]) < 1e-7
    graph.replay()
    torch.cuda.synchronize()
    for m, r in enumerate(refs):
        assert_tick_equal(pop.members[m], r.snaps[17], f"member {m} after the third replay")
        assert_final_equal(pop.members[m], r.eng, f"member {m} end")
    assert pop.handoff_errors() == [0, 0, 0]


def _trainer(sw, seed, root, **hp):
    env = sw.make_env(scenario=sw.GoToPositionScenario(), num_envs=1, continuous_actions=False, wrapper=None,
                      max_steps=6, dict_spaces=True, n_agents=5, seed=seed)
    sw.set_seed(seed)
    return sw.DQNTrainer(env, seed, os.path.join(root, "models"), os.path.join(root, "stats"), "GoTo", batch_size=4,
                         replay_capacity=1000, **hp)


def test_population_trainer_with_different_optimizers_and_eps_schedules(tmp_path):
    sw = _sw()
    seeds = (0, 1)
    hps = (dict(lr=1e-3, update_target_every=2), dict(lr=3e-3, update_target_every=3))
    eps = dict(epsilon=[0.99, 0.5], epsilon_decay=[0.01, 0.7], min_epsilon=[0.05, 0.2])
    lone_root, pop_root = str(tmp_path / "lone"), str(tmp_path / "pop")
    lone_tr = [_trainer(sw, s, lone_root, **hp) for s, hp in zip(seeds, hps)]
    for m, t in enumerate(lone_tr):
        t.train_model({"episodes": 3, **{k: v[m] for k, v in eps.items()}})
    pop_tr = [_trainer(sw, s, pop_root, **hp) for s, hp in zip(seeds, hps)]
    trainer = sw.PopulationTrainer(pop_tr)
    assert trainer.population.per_member_hp is True
    trainer.train_model({"episodes": 3, **eps})
    for s, a, b in zip(seeds, lone_tr, pop_tr):
        assert a.engine.read_ctrl()["adam_step"] == b.engine.read_ctrl()["adam_step"] >= 2
        assert a.engine.read_ctrl()["eps"] == b.engine.read_ctrl()["eps"]
        assert a.episode_losses == b.episode_losses and len(a.episode_losses) == 3
        # 3 episodes end no 10-episode window: episode_rewards is empty in both, the sums behind it are not
        assert [float(x) for x in a.episode_rewards] == [float(x) for x in b.episode_rewards]
        assert [float(x) for x in a.rewards_buffer] == [float(x) for x in b.rewards_buffer] and len(a.rewards_buffer) == 3
        name = f"experiment_GoTo-seed_{s}.pth"
        sa = torch.load(os.path.join(lone_root, "models", name))
        sb = torch.load(os.path.join(pop_root, "models", name))
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"seed {s}: {k}"
    # the two members really trained differently (not one optimizer for both)
    assert lone_tr[0].engine.read_ctrl()["eps"] != lone_tr[1].engine.read_ctrl()["eps"]
