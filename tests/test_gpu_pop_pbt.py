"""Population-based training on the GPU (swarm_pop_exploit, SwarmPopulation.exploit / sync_hp,
PopulationTrainer's pbt_every).  ``restate`` below is a numpy restatement of the semantics stated in
include/swarm_hip.h (ranking, Philox draws, explore arithmetic); every comparison with it, and every
other comparison in this file, is bit for bit.  Shapes: GoTo, 4 agents, 4 envs, batch 4, a ring of
8 slots, 6 members unless said otherwise: the smallest at which a pending step, a ring that wraps
and the three rank classes (parents, middle, children) all occur.  Hand-off error words are 0
throughout."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle.philox import philox4x32, seed_key, u01, uniform_int
from tests.test_gpu_population import FINAL_FIELDS, TICK_FIELDS

pytestmark = pytest.mark.gpu

STREAM_PBT = 5
N_PARAMS = 1673
KW = dict(scenario="GoTo", n_agents=4, n_envs=4, batch=4, replay_capacity=8 * 4, eps=0.3, update_target_every=5)
# the control words that go from parent to child: adam_step, loss, grad_norm, trained, beta_pow[4],
# adam_step_size, adam_inv_bc2, one_m_beta1, one_m_beta2
OPT_WORDS = [3, 5, 6, 7, 10, 11, 12, 13, 14, 15, 24, 25]
OWN_WORDS = [w for w in range(32) if w not in OPT_WORDS]
# everything a member owns on the device
BUFS = ("_lrn", "grad", "ctrl", "rep_s", "rep_s1", "rep_r", "rep_a", "_state_buf", "slabs", "tick_ws", "samples")
LRS = [1e-3, 2e-3, 5e-4, 3e-3, 1.5e-3, 8e-4]
GAMMAS = [0.99, 0.95, 0.9, 0.97, 0.8, 0.85]
SCORES6 = [0.3, -1.0, 2.0, 0.1, 5.0, -3.0]   # ranks: 4, 2, 0, 3, 1, 5: with n_replace = 2 parents {4, 2}, children {1, 5}
BOTH = ("lr", "gamma")


def _sw():
    import swarm_amd
    return swarm_amd


def _L():
    import swarm_amd._lib as L
    return L


# ------------------------------------------------------------------ the restatement
def _copy_row(r):
    return type(r).from_buffer_copy(_row_bytes(r))


def _row_bytes(r) -> bytes:
    return ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r))


def ranks(score) -> list:
    s = np.asarray(score, dtype=np.float32).copy()
    s[np.isnan(s)] = -np.inf
    idx = np.arange(len(s))
    return [int(np.sum((s > s[m]) | ((s == s[m]) & (idx < m)))) for m in range(len(s))]


def restate(score, rows, *, round, n_replace, seed=0, fields=("lr",), perturb=(0.8, 1.2), lr_bounds=(1e-6, 1e-1),
            gamma_bounds=(0.0, 0.9999)):
    """(parent [P], rows [P] of SwarmAdamCfg) after one round on `rows`"""
    P = len(rows)
    rank = ranks(score)
    assert sorted(rank) == list(range(P))
    by_rank = [rank.index(r) for r in range(P)]
    k0, k1 = seed_key(seed)
    lo, hi = np.float32(perturb[0]), np.float32(perturb[1])
    parent, out = list(range(P)), [_copy_row(r) for r in rows]
    for m in range(P):
        if rank[m] < P - n_replace:
            continue
        w = [int(x) for x in philox4x32(round, m, STREAM_PBT, 0, k0, k1)]
        p = by_rank[int(uniform_int(w[0], n_replace))]
        parent[m] = p
        row = _copy_row(rows[p])
        if "lr" in fields:
            f = lo if u01(w[1]) < np.float32(0.5) else hi
            base = row.lr_d if row.lr_d != 0.0 else float(row.lr)
            x = min(max(base * float(f), float(lr_bounds[0])), float(lr_bounds[1]))   # one double product
            row.lr_d, row.lr = x, float(np.float32(x))
        if "gamma" in fields:
            f = lo if u01(w[2]) < np.float32(0.5) else hi
            g = np.float32(1.0) - (np.float32(1.0) - np.float32(row.gamma)) * f     # fp32, two roundings
            g = min(max(g, np.float32(gamma_bounds[0])), np.float32(gamma_bounds[1]))
            row.gamma = float(g)
        out[m] = row
    return parent, out


# ------------------------------------------------------------------ helpers
def bits(t):
    return t.contiguous().view(torch.uint8)


def same(a, b) -> bool:
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def read_rows(pop) -> list:
    L = _L()
    raw, n = pop._hp_table.cpu().numpy().tobytes(), ctypes.sizeof(L.SwarmAdamCfg)
    return [L.SwarmAdamCfg.from_buffer_copy(raw[m * n:(m + 1) * n]) for m in range(pop.P)]


def snapshot(pop) -> list:
    return [{f: getattr(e, f).clone() for f in BUFS} for e in pop.members]


def assert_member_unchanged(e, snap, what):
    for f in BUFS:
        assert same(getattr(e, f), snap[f]), f"{what}: {f}"


def frac_for(P: int, n: int) -> float:
    """a frac <= 0.5 with int(frac * P) == n"""
    for frac in (n / P, min((n + 0.5) / P, 0.5)):
        if int(frac * P) == n and frac <= 0.5:
            return frac
    raise AssertionError((P, n))


def population(P, ticks, **over):
    kw = dict(KW, **over)
    pop = _sw().SwarmPopulation(seeds=list(range(P)), **kw)
    pop.reset(0)
    for _ in range(ticks):
        pop.train_tick(full_out=True)
    return pop


def device_score(pop, score):
    return torch.tensor(score, dtype=torch.float32, device=pop.device)


def check_plan(pop, score, n_replace, what, **kw):
    """one exploit through the public call against the restatement: parent[] and every row"""
    before = read_rows(pop)
    want_parent, want_rows = restate(score, before, n_replace=n_replace, **kw)
    parent = pop.exploit(device_score(pop, score), frac=frac_for(pop.P, n_replace), **kw)
    assert parent.dtype == torch.int32 and parent.tolist() == want_parent, what
    got = read_rows(pop)
    for m in range(pop.P):
        assert _row_bytes(got[m]) == _row_bytes(want_rows[m]), f"{what}: row {m}"
        # sync=True: the member's host hp is the row, with its own batch / world_size / flags
        hp = pop.members[m].hp
        assert (hp.lr, hp.lr_d, hp.gamma, hp.batch) == (got[m].lr, got[m].lr_d, got[m].gamma, KW["batch"]), what
    assert pop.per_member_hp is True and pop._hp_stale is False
    return want_parent


_POPS = {}


def plan_population(P):
    """one population per size, two ticks in: the plan cases run on it one after another (each
    case restates from the rows as the case before left them)"""
    if P not in _POPS:
        over = dict(lr=[1e-3 * (1 + m % 7) for m in range(P)], gamma=[0.99 - 0.01 * (m % 5) for m in range(P)])
        _POPS[P] = population(P, 2, **over)
    return _POPS[P]


# ------------------------------------------------------------------ 1. plan
@pytest.mark.parametrize("P", [1, 2, 5, 6, 64])
def test_plan_sizes_and_replace_counts(P):
    pop = plan_population(P)
    rng = np.random.default_rng(100 + P)
    rnd = 0
    for n_replace in sorted({0, min(1, P // 2), P // 2}):
        for fields in (BOTH, ("lr",), ("gamma",), ()):
            score = rng.standard_normal(P).astype(np.float32).tolist()
            snap = snapshot(pop) if n_replace == 0 else None
            parent = check_plan(pop, score, n_replace, f"P {P} n_replace {n_replace} {fields}", round=rnd, seed=11 + P,
                                fields=fields)
            assert sum(p != m for m, p in enumerate(parent)) == n_replace
            if n_replace == 0:   # nothing but parent[] is written: every buffer of every member keeps its bits
                for m, e in enumerate(pop.members):
                    assert_member_unchanged(e, snap[m], f"P {P} member {m}")
            rnd += 1
    assert pop.handoff_errors() == [0] * P


def test_plan_ties_and_special_scores():
    pop = plan_population(6)
    nan, inf = math.nan, math.inf
    cases = [
        ("all equal", [1.5] * 6, 3),                       # ranks are the indices
        ("all equal, one child", [0.0] * 6, 1),
        ("tie across the parent / middle boundary", [5.0, 5.0, 5.0, 1.0, 0.0, 2.0], 2),   # parents 0, 1; 2 is middle
        ("tie across the middle / child boundary", [5.0, 1.0, 1.0, 1.0, 1.0, 9.0], 2),    # children 3, 4
        ("-0.0 == 0.0", [0.0, -0.0, 0.0, -0.0, 1.0, -1.0], 3),
        ("nan, inf, -inf", [nan, inf, -inf, 0.0, nan, 1.0], 3),    # nan == -inf: children 0, 2, 4 by index
        ("nan, inf, -inf, two children", [nan, inf, -inf, 0.0, nan, 1.0], 2),
        ("all nan", [nan] * 6, 3),
        ("all +inf", [inf] * 6, 2),
    ]
    assert ranks(cases[5][1]) == [3, 0, 4, 2, 5, 1]
    assert ranks(cases[2][1]) == [0, 1, 2, 4, 5, 3]
    for i, (what, score, n_replace) in enumerate(cases):
        check_plan(pop, score, n_replace, what, round=50 + i, seed=(9 << 32) | 3, fields=BOTH)
    assert pop.handoff_errors() == [0] * 6


def test_plan_clamps_and_a_parent_row_without_lr_d():
    pop = plan_population(6)
    rows = read_rows(pop)
    # bounds that clamp: every row's lr and gamma lie outside them on one side or the other
    lrs, gs = [r.lr_d for r in rows], [r.gamma for r in rows]
    for i, (lr_b, g_b) in enumerate([((2 * max(lrs), 4 * max(lrs)), (0.99995, 0.99999)),      # both floors bite
                                     ((min(lrs) / 8, min(lrs) / 4), (0.0, 0.05)),              # both ceilings bite
                                     ((1e-6, 1e-1), (0.0, 0.9999))]):
        rows = read_rows(pop)
        parent = check_plan(pop, SCORES6, 2, f"clamp {i}", round=70 + i, fields=BOTH, lr_bounds=lr_b, gamma_bounds=g_b)
        got = read_rows(pop)
        for c in (1, 5):
            assert parent[c] in (4, 2)
            if i < 2:   # the clamp, not the product, decided
                assert got[c].lr_d == lr_b[i] and got[c].gamma == np.float32(g_b[i])
    # a parent row whose lr_d is 0 ("use the float field"): the child's lr_d is formed from (double)lr
    rows = read_rows(pop)
    rows[3].lr_d = 0.0
    pop._hp_table[3].copy_(torch.frombuffer(bytearray(_row_bytes(rows[3])), dtype=torch.uint8))
    score = [0.0, 1.0, 2.0, 9.0, 3.0, -1.0]   # member 3 is the one parent, member 5 the one child
    parent = check_plan(pop, score, 1, "lr_d == 0", round=80, fields=("lr",))
    assert parent == [0, 1, 2, 3, 4, 3]
    got = read_rows(pop)
    assert got[3].lr_d == 0.0 and got[5].lr_d in (float(rows[3].lr) * float(np.float32(0.8)),
                                                  float(rows[3].lr) * float(np.float32(1.2)))
    assert got[5].lr == np.float32(got[5].lr_d)


# ------------------------------------------------------------------ 2. copy
def test_copy_moves_the_learner_and_nothing_else():
    pop = population(6, 12, lr=LRS, gamma=GAMMAS)
    ctrl = pop.ctrl.cpu()
    assert ctrl[:, 7].tolist() == [1] * 6 and int(ctrl[:, 3].min()) >= 2    # a step is pending; steps were taken
    assert int(ctrl[:, 2].min()) == 8 and ctrl[:, 0].tolist() == [12] * 6   # the ring wrapped
    for a in range(6):
        e = pop.members[a]
        assert not torch.equal(e.params, e.target)
        for b in range(a):
            assert not any(torch.equal(getattr(e, f), getattr(pop.members[b], f)) for f in ("params", "adam_m", "adam_v"))
    snap, rows = snapshot(pop), read_rows(pop)
    parent = pop.exploit(device_score(pop, SCORES6), round=0, seed=5, frac=frac_for(6, 2), fields=BOTH).tolist()
    want_parent, want_rows = restate(SCORES6, rows, round=0, seed=5, n_replace=2, fields=BOTH)
    assert parent == want_parent and [m for m in range(6) if parent[m] != m] == [1, 5]
    assert set(parent[c] for c in (1, 5)) <= {4, 2}
    got = read_rows(pop)
    for m, e in enumerate(pop.members):
        p = parent[m]
        assert _row_bytes(got[m]) == _row_bytes(want_rows[m]), m
        if p == m:   # parents and middle members: not written at all
            assert_member_unchanged(e, snap[m], f"member {m}")
            continue
        assert same(e._lrn[:, :N_PARAMS], snap[p]["_lrn"][:, :N_PARAMS]), f"child {m}: learner rows"
        assert same(e._lrn[:, N_PARAMS:], snap[m]["_lrn"][:, N_PARAMS:]), f"child {m}: the rows' padding"
        assert same(e.grad, snap[p]["grad"]), f"child {m}: grad"
        assert same(e.ctrl[OPT_WORDS], snap[p]["ctrl"][OPT_WORDS]), f"child {m}: the optimizer's control words"
        assert same(e.ctrl[OWN_WORDS], snap[m]["ctrl"][OWN_WORDS]), f"child {m}: its own control words"
        for f in ("rep_s", "rep_s1", "rep_r", "rep_a", "_state_buf", "slabs", "tick_ws", "samples"):
            assert same(getattr(e, f), snap[m][f]), f"child {m}: {f}"
        # the copy mattered: the child's own learner was another
        assert not same(snap[m]["_lrn"], snap[p]["_lrn"]) and not same(snap[m]["grad"], snap[p]["grad"])
    assert pop.handoff_errors() == [0] * 6


# ------------------------------------------------------------------ 3. meaning
def host_exploit(pop, score, **kw):
    """The same round done with what the population offered before swarm_pop_exploit: the plan on
    the host (the restatement), tensor copies of the same buffers, set_member_hp."""
    n_replace = kw.pop("n_replace")
    parent, rows = restate(score, read_rows(pop), n_replace=n_replace, **kw)
    for c, p in enumerate(parent):
        if p == c:
            continue
        ce, pe = pop.members[c], pop.members[p]
        ce._lrn[:, :N_PARAMS].copy_(pe._lrn[:, :N_PARAMS])
        ce.grad.copy_(pe.grad)
        ce.ctrl[OPT_WORDS] = pe.ctrl[OPT_WORDS]
        r = rows[c]
        pop.set_member_hp(c, lr=r.lr_d, gamma=r.gamma, betas=(r.beta1_d, r.beta2_d), adam_eps=r.eps, max_norm=r.max_norm,
                          update_target_every=r.update_target_every)
    return parent


@pytest.mark.parametrize("flushed", [False, True], ids=["pending_step", "after_flush"])
def test_exploit_means_host_copies_plus_set_member_hp(flushed):
    A, B = (population(6, 12, lr=LRS, gamma=GAMMAS) for _ in range(2))
    for pop in (A, B):
        assert pop.ctrl[:, 7].tolist() == [1] * 6
        if flushed:
            pop.flush()
            assert pop.ctrl[:, 7].tolist() == [0] * 6
    snap_b = snapshot(B)
    for m in range(6):
        assert_member_unchanged(A.members[m], snap_b[m], f"member {m} before the round")
    kw = dict(round=3, seed=(1 << 40) | 17, fields=BOTH, perturb=(0.5, 1.5))
    pa = A.exploit(device_score(A, SCORES6), frac=frac_for(6, 2), **kw).tolist()
    pb = host_exploit(B, SCORES6, n_replace=2, **kw)
    assert pa == pb and sorted(m for m in range(6) if pa[m] != m) == [1, 5]
    assert same(A._hp_table, B._hp_table)
    assert A.per_member_hp is True and B.per_member_hp is True
    for m in range(6):
        assert _row_bytes(A.members[m].hp) == _row_bytes(B.members[m].hp), f"member {m}: host hp after sync_hp"
    for t in range(6):
        A.train_tick(full_out=True)
        B.train_tick(full_out=True)
        for m in range(6):
            for f in TICK_FIELDS:
                assert same(getattr(A.members[m], f), getattr(B.members[m], f)), f"tick {t} member {m}: {f}"
    for m in range(6):
        for f in FINAL_FIELDS:
            assert same(getattr(A.members[m], f), getattr(B.members[m], f)), f"end, member {m}: {f}"
    # the children really went on from their parents: they took optimizer steps with the explored rows
    ctrl = A.ctrl.cpu()
    assert ctrl[:, 0].tolist() == [18] * 6 and ctrl[:, 7].tolist() == [1] * 6
    A.flush()
    B.flush()
    for m in range(6):
        for f in ("params", "adam_m", "adam_v", "target", "ctrl"):
            assert same(getattr(A.members[m], f), getattr(B.members[m], f)), f"flushed, member {m}: {f}"
    assert A.handoff_errors() == B.handoff_errors() == [0] * 6


# ------------------------------------------------------------------ 4. captured
def test_captured_round_replays_as_the_eager_one():
    """One hipGraph of {6 ticks, evaluate, the score's reduction, exploit(sync=False)}, replayed
    twice, against the same sequence run eagerly twice.  `round` is a kernel argument and so frozen
    into the graph: both replays run round 0, and so does the eager side (a trainer that wants a
    new round per exploit calls it outside the graph, as PopulationTrainer does)."""
    sw = _sw()
    pops = [population(6, 0, lr=LRS, gamma=GAMMAS) for _ in range(2)]
    scores = [torch.zeros(6, device=p.device) for p in pops]

    def sequence(pop, score):
        for _ in range(6):
            pop.train_tick(full_out=True)
        res = pop.evaluate(4, 5, seed=77)
        torch.sum(res["reward"], dim=(1, 2), out=score)
        pop.exploit(score, round=0, seed=3, frac=frac_for(6, 2), fields=BOTH, sync=False)

    for pop in pops:
        pop.per_member_hp = True     # before the capture: the rows will change
        pop.evaluate(4, 5, seed=77)   # builds the evaluation's buffers and table once, outside the graph
    eager, cap = pops
    graph = cap.capture(1, lambda: sequence(cap, scores[1]))
    assert cap.ctrl[:, 0].tolist() == [0] * 6 and cap._hp_stale   # capture ran nothing; the host hp is marked behind
    parents = []
    for rep in range(2):
        sequence(eager, scores[0])
        graph.replay()
        torch.cuda.synchronize()
        assert same(scores[0], scores[1]) and same(eager.parent, cap.parent), rep
        parents.append(cap.parent.tolist())
        assert sum(p != m for m, p in enumerate(parents[-1])) == 2
        assert same(eager._hp_table, cap._hp_table)
        for m in range(6):
            for f in TICK_FIELDS + FINAL_FIELDS:
                assert same(getattr(eager.members[m], f), getattr(cap.members[m], f)), f"replay {rep} member {m}: {f}"
    assert cap.ctrl[:, 0].tolist() == [12] * 6
    # the device rows are ahead of the host hp until sync_hp()
    rows = read_rows(cap)
    assert any(_row_bytes(cap._row(e)) != _row_bytes(r) for e, r in zip(cap.members, rows))
    cap.sync_hp()
    assert not cap._hp_stale
    # each member's own flush now agrees with a lone engine given the same row and state
    for m, e in enumerate(cap.members):
        r = rows[m]
        assert (e.hp.lr_d, e.hp.gamma, e.hp.batch, e.hp.world_size) == (r.lr_d, r.gamma, KW["batch"], 1)
        lone = sw.SwarmEngine(seed=m, **KW)
        lone.set_hp(lr=r.lr_d, gamma=r.gamma, betas=(r.beta1_d, r.beta2_d), adam_eps=r.eps, max_norm=r.max_norm,
                    update_target_every=r.update_target_every)
        lone._lrn.copy_(e._lrn)
        lone.grad.copy_(e.grad)
        lone.ctrl.copy_(e.ctrl)
        assert int(e.ctrl[7]) == 1
        lone.flush()
        e.flush()
        for f in ("params", "adam_m", "adam_v", "target", "ctrl"):
            assert same(getattr(e, f), getattr(lone, f)), f"member {m} flush: {f}"
        assert int(e.ctrl[7]) == 0
    assert cap.handoff_errors() == eager.handoff_errors() == [0] * 6


# ------------------------------------------------------------------ 5. trainer
def _trainers(sw, root, seeds=(0, 1, 2, 3)):
    out = []
    for seed in seeds:
        env = sw.make_env(scenario=sw.GoToPositionScenario(), num_envs=1, continuous_actions=False, wrapper=None,
                          max_steps=10, dict_spaces=True, n_agents=5, seed=seed)
        sw.set_seed(seed)
        out.append(sw.DQNTrainer(env, seed, os.path.join(root, "models"), os.path.join(root, "stats"), "GoTo",
                                 batch_size=4, replay_capacity=1000, lr=1e-3 * (1 + seed)))
    return out


def _run(sw, root, **extra):
    config = {"epsilon": 0.99, "epsilon_decay": 0.01, "min_epsilon": 0.05, "episodes": 4, "eval_every": 2,
              "eval_envs": 4, **extra}
    trainers = _trainers(sw, root)
    pt = sw.PopulationTrainer(trainers)
    pt.train_model(config)
    assert pt.population.handoff_errors() == [0] * 4
    return trainers


def _files(root, seed) -> dict:
    name = f"experiment_GoTo-seed_{seed}"
    out = {k: os.path.join(root, "stats", name + k) for k in (".csv", "-eval.csv", "-pbt.csv")}
    out[".pth"] = os.path.join(root, "models", name + ".pth")
    return out


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _same_models(a, b) -> bool:
    sa, sb = torch.load(a), torch.load(b)
    return list(sa) == list(sb) and all(same(sa[k], sb[k]) for k in sa)


def test_trainer_rounds_are_reproducible_and_follow_the_logged_rewards(tmp_path):
    sw = _sw()
    roots = [str(tmp_path / n) for n in ("a", "b")]
    pbt = dict(seed=21, fields=BOTH)
    runs = [_run(sw, r, pbt_every=2, pbt=pbt) for r in roots]
    for seed in range(4):
        fa, fb = _files(roots[0], seed), _files(roots[1], seed)
        for k in (".csv", "-eval.csv", "-pbt.csv"):
            assert _read(fa[k]) == _read(fb[k]), (seed, k)
        assert _same_models(fa[".pth"], fb[".pth"]), seed
        assert _read(fa["-pbt.csv"]).startswith(b"Episode,Parent,lr,gamma\r\n")
    trainers = runs[0]
    assert all([r[0] for r in t.pbt_rows] == [1, 3] and len(t.eval_rows) == 2 for t in trainers)
    for rnd in range(2):
        # the logged evaluation rewards are the device scores divided by envs * ticks: the same order,
        # unless two differ by no more than that division's rounding, which the guard excludes (two
        # that are equal come from equal rollouts, young greedy policies that all push one way, and
        # have equal device scores: the lower index ranks better in both)
        score = [t.eval_rows[rnd][1] for t in trainers]
        print("round", rnd, "logged evaluation rewards", score)
        scale = 1e-5 * max(abs(s) for s in score)
        assert all(a == b or abs(a - b) > scale for i, a in enumerate(score) for b in score[:i]), score
        rank = ranks(score)
        child, best = rank.index(3), rank.index(0)
        want = list(range(4))
        want[child] = best   # n_replace = int(0.25 * 4) = 1: the one parent is rank 0, whatever the draw
        assert [t.pbt_rows[rnd][1] for t in trainers] == want, rnd
        for m, t in enumerate(trainers):
            lr, gamma = t.pbt_rows[rnd][2:]
            if m != child:
                prev = t.pbt_rows[rnd - 1][2:] if rnd else (1e-3 * (1 + m), float(np.float32(0.99)))
                assert (lr, gamma) == prev, (rnd, m)
        src = trainers[best].pbt_rows[rnd]
        got = trainers[child].pbt_rows[rnd]
        assert got[2] in (src[2] * float(np.float32(0.8)), src[2] * float(np.float32(1.2)))
        assert got[3] != src[3]
    # the engines' host hp at the end are the last round's rows
    for t in trainers:
        assert (t.engine.hp.lr_d, t.engine.hp.gamma) == tuple(t.pbt_rows[-1][2:])


def test_trainer_without_pbt_is_the_plain_evaluation_run(tmp_path):
    """No pbt_every: the files of a plain eval_every run and no -pbt.csv.  pbt_every with frac = 0
    (rounds that replace nobody; the population ticks through the per-member entry points from the
    start) writes the same bytes in all of them, plus a -pbt.csv of unchanged rows."""
    sw = _sw()
    roots = [str(tmp_path / n) for n in ("plain", "plain2", "idle")]
    _run(sw, roots[0])
    _run(sw, roots[1])
    idle = _run(sw, roots[2], pbt_every=2, pbt=dict(frac=0.0))
    for seed in range(4):
        fp, fq, fi = (_files(r, seed) for r in roots)
        assert not os.path.exists(fp["-pbt.csv"]) and not os.path.exists(fq["-pbt.csv"])
        for k in (".csv", "-eval.csv"):
            assert _read(fp[k]) == _read(fq[k]) == _read(fi[k]), (seed, k)
        assert _same_models(fp[".pth"], fq[".pth"]) and _same_models(fp[".pth"], fi[".pth"]), seed
    for m, t in enumerate(idle):
        assert t.pbt_rows == [(e, m, 1e-3 * (1 + m), float(np.float32(0.99))) for e in (1, 3)]
