"""Optimizer hyper-parameters against torch, not only path against path.

The population sweeps, set_hp / set_member_hp and PBT rest on the learner computing the right thing
at hyper-parameters other than the reference's defaults; every other reference comparison of the
suite runs at the defaults and every other hyper-parameter test compares two of the project's own
paths.  Here:

- the optimizer step (swarm_adam_step, and swarm_adam_flush on a pending step) on injected
  gradients, six consecutive steps per case of tests/hp_cases.py, each step against
  clip_grad_norm_ + torch.optim.Adam from the GPU's own p, m, v before it (_adam_check of
  tests/test_gpu_parity_large.py at the case's values), the two paths bit-equal;
- update_target_every: when the target row is written, and with what;
- the bias-correction scalars of the control block over 3,000 steps against Python floats;
- gamma in the TD kernel against the oracle's autograd at the smallest shape of each kernel family;
- three engines (fused tick, 3-launch tick, unfused) through a mid-run set_hp of every field;
- the first optimizer step after set_hp (the transition step) against its restatement.

Bounds: tests/hp_cases.py (the project's bounds, or 2x the fp32 restatement's measured rounding
noise on the same inputs where that is larger); tests/test_hp_reference_host.py checks on the CPU
that a kernel which ignored a field would miss them by more than 10x.
"""
import numpy as np
import pytest
import torch

from oracle import swarm_oracle as O
from tests import hp_cases as H
from tests.conftest import assert_close_ulp, record
from tests.test_gpu_parity import LOSS_ULP, _fill_replay, _params
from tests.test_gpu_parity_large import _adam_check, _grad_bound_check, oracle_grad_orders

pytestmark = pytest.mark.gpu

NP = O.N_PARAMS
LOSS_WORD = 3.0
# ctrl's optimizer words: adam_step, beta_pow[4], adam_step_size, adam_inv_bc2, one_m_beta1/2
OPT_WORDS = [3, 10, 11, 12, 13, 14, 15, 24, 25]


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


@pytest.fixture(scope="module")
def p_init(golden_weights):
    return torch.tensor(golden_weights["go_to"][0])


def _tiny(sw, p, hp):
    """A learner that only ever runs optimizer steps: no TD batch, filled_slots large enough."""
    return sw.SwarmEngine("GoTo", 2, 2, seed=1, params=p, batch=2, replay_capacity=4, **hp)


def _inject(eng, g):
    eng.grad[:NP].copy_(g.cuda())
    eng.grad[NP] = LOSS_WORD
    eng.grad_written()


def _step(eng, path):
    """One optimizer step: swarm_adam_step, or swarm_adam_flush on a step declared pending."""
    from swarm_amd._lib import CTRL
    if path == "step":
        eng.adam()
    else:
        eng.ctrl[CTRL["trained"]] = 1
        eng.flush()


def _pmv(eng):
    torch.cuda.synchronize()
    return eng.params.cpu().clone(), eng.adam_m.cpu().clone(), eng.adam_v.cpu().clone()


@pytest.mark.parametrize("name", list(H.CASES))
def test_optimizer_step_against_torch(sw, p_init, name):
    """Six steps from a fresh control block through swarm_adam_step and through swarm_adam_flush,
    each against torch from the GPU's own state before it, and the two paths bit for bit."""
    hp = H.case_hp(name)
    lr, (b1, b2), eps, W = hp["lr"], hp["betas"], hp["adam_eps"], hp["world_size"]
    engs = {path: _tiny(sw, p_init, hp) for path in ("step", "flush")}
    steps = {path: [] for path in engs}
    for s in range(H.N_STEPS):
        g = H.synthetic_grad(name, s)
        mn = H.step_max_norm(name, s, g, W)
        for path, eng in engs.items():
            eng.set_hp(max_norm=mn)
            p0, m0, v0 = _pmv(eng)
            _inject(eng, g)
            _step(eng, path)
            p1, m1, v1 = _pmv(eng)
            c = eng.read_ctrl()
            assert c["adam_step"] == s + 1 and c["trained"] == 0
            if path == "step":
                assert c["tick"] == s + 1
                assert c["loss"] == float(np.float32(np.float32(LOSS_WORD) / np.float32(4.0)) / np.float32(W))
            steps[path].append(dict(p0=p0, m0=m0, v0=v0, g=g, mn=mn, p=p1, m=m1, v=v1, norm=c["grad_norm"]))
        a, b = steps["step"][-1], steps["flush"][-1]
        assert all(torch.equal(a[k], b[k]) for k in ("p", "m", "v")) and a["norm"] == b["norm"], (name, s)
        assert torch.equal(engs["step"].ctrl.cpu()[OPT_WORDS], engs["flush"].ctrl.cpu()[OPT_WORDS]), (name, s)
    # the bound of the case: the project's, or 2x the fp32 restatement's noise on these very inputs
    noise = dict.fromkeys(H.PROJECT_ULP, 0.0)
    for s, st in enumerate(steps["step"]):
        sc = H.adam_scalars(lr, b1, b2, s)
        r64 = H.adam_ref64(st["p0"], st["g"], st["m0"], st["v0"], sc, eps, st["mn"], W)
        st["r64"], st["sc"] = r64, sc
        n = H.ulp_errors(H.adam_np32(st["p0"], st["g"], st["m0"], st["v0"], sc, eps, st["mn"], W), r64,
                         H.scales(st["p0"], st["m0"], st["v0"], r64, sc, lr))
        noise = {k: max(noise[k], n[k]) for k in noise}
    bound = H.bounds_from_noise(noise)
    record(f"hp {name}: fp32 restatement vs float64 on the GPU's inputs (ulp)", noise)
    record(f"hp {name}: asserted bounds (ulp)", bound)
    for s, st in enumerate(steps["step"]):   # the flush path's results are these, bit for bit
        if lr == 0.0:
            assert torch.equal(st["p"], st["p0"]), "lr = 0 leaves the weights bit for bit"
            assert not torch.equal(st["m"], st["m0"]) and not torch.equal(st["v"], st["v0"])
        _adam_check(f"hp {name} step {s}", st["p"], st["m"], st["v"], st["p0"], st["g"], st["m0"], st["v0"], s,
                    norm_gpu=st["norm"], lr=lr, b1=b1, b2=b2, eps=eps, max_norm=st["mn"], world_size=W, tol=bound,
                    general=True)
        # what the case claims of its own inputs, on the GPU's state (tests/test_hp_reference_host.py)
        coef = st["mn"] / (st["norm"] + 1e-6)
        root = (st["v"].double() / st["sc"]["bc2"]).sqrt()
        if name == "adam_eps=1e-3":
            assert float((eps > root).double().mean()) > 0.01
        elif name == "adam_eps=1e-12":
            assert float((eps < 0.01 * root[root > 0]).double().mean()) > 0.99
        elif name == "max_norm=1e-3":
            assert coef < 1.0
        elif name == "max_norm=1e3":
            assert coef > 1.0
        elif name == "max_norm=edge":
            assert (1.0 < coef < 1.01) if s % 2 == 0 else (0.99 < coef < 1.0)
        elif name == "world_size=2":
            assert 0.5 < st["norm"] < 1.0, "the halved gradient is not clipped, the whole one would be"


@pytest.mark.parametrize("every", [1, 2, 5])
def test_update_target_every(sw, p_init, every):
    """After each swarm_adam_step the target row is the new weights, bit for bit, exactly when
    (tick + 1) % update_target_every == 0, and untouched otherwise."""
    hp = dict(H.DEFAULTS, update_target_every=every)
    eng = _tiny(sw, p_init, hp)
    tgt = eng.target.cpu().clone()
    synced = 0
    for s in range(10):
        p0 = eng.params.cpu().clone()
        tick = eng.read_ctrl()["tick"]
        _inject(eng, H.synthetic_grad("update_target_every", s, kind="std"))
        eng.adam()
        torch.cuda.synchronize()
        p1 = eng.params.cpu().clone()
        assert float((p1 != p0).double().mean()) > 0.9, "the step moved the weights: a sync is visible"
        if (tick + 1) % every == 0:
            assert torch.equal(eng.target.cpu(), p1), (every, s)
            tgt, synced = p1, synced + 1
        else:
            assert torch.equal(eng.target.cpu(), tgt), (every, s)
    assert synced == 10 // every


def _ulps(got, ref):
    ref32 = np.float32(ref)
    return abs(float(got) - float(ref32)) / float(np.spacing(ref32))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9), (0.99, 0.9999)])
def test_bias_correction_scalars_over_3000_steps(sw, p_init, betas):
    """ctrl's adam_step_size and adam_inv_bc2 after s steps are the scalars of step s + 1: against
    lr / (1 - b1**(s+1)) and 1 / sqrt(1 - b2**(s+1)) in Python floats.  Derived bounds: the running
    double product is within s * 2^-53 relative of b**s and the subtraction amplifies that by at most
    1 / (1 - b), so the correctly rounded fp32 value or its neighbour results: <= 1 ulp for the step
    size, <= 2 ulp for adam_inv_bc2 (two roundings).  (0.5, 0.9): b**s underflows to 0 past
    s ~ 1075 and the scalars become lr and 1."""
    from swarm_amd._lib import CTRL
    lr = 1e-3
    eng = _tiny(sw, p_init, dict(H.DEFAULTS, betas=betas))
    _inject(eng, H.synthetic_grad("bias corrections", 0, kind="std"))
    looks = (0, 1, 2, 10, 100, 1000, 1100, 3000)
    s = 0
    for look in looks:
        while s < look:
            eng.adam()
            s += 1
        c = eng.ctrl.cpu()
        assert int(c[CTRL["adam_step"]]) == s
        f = c.view(torch.float32)
        e1 = _ulps(f[CTRL["adam_step_size"]], lr / (1.0 - betas[0] ** (s + 1)))
        e2 = _ulps(f[CTRL["adam_inv_bc2"]], 1.0 / np.sqrt(1.0 - betas[1] ** (s + 1)))
        record(f"hp bias corrections betas={betas} after {s} steps (ulp)", {"adam_step_size": e1, "adam_inv_bc2": e2})
        assert e1 <= 1.0 and e2 <= 2.0, (betas, s, e1, e2)
    if betas == (0.5, 0.9):
        assert float(f[CTRL["adam_step_size"]]) == float(np.float32(lr))
    assert torch.isfinite(eng.params).all()


# ------------------------------------------------------------------ gamma in the TD kernel
TD_SHAPES = [("go_to", 5, 7, "complete", 0, "gat"), ("obstacle_avoidance", 12, 24, "knn", 5, "gat"),
             ("go_to", 8, 32, "complete", 0, "gcn"), ("go_to", 20, 9, "complete", 0, "gat")]


def _td_case(sw, golden_weights, scen, N, S, graph, k, conv, gamma, tgt_seed=6):
    B = 16
    cap = max(4, -(-S // B))
    p = _params(golden_weights, scen, 5)
    tgt = _params(golden_weights, scen, tgt_seed)
    eng = sw.SwarmEngine(scen, N, B, seed=2, params=p, batch=S, replay_capacity=cap * B, update_target_every=1000,
                         graph=graph, knn_k=max(k, 1), conv=conv, gamma=gamma)
    eng.target.copy_(tgt.cuda())
    _fill_replay(eng, S)
    idx = torch.randperm(cap * B, generator=torch.Generator().manual_seed(S))[:S].to(torch.int32)
    eng.td_grad(sample_in=idx.cuda())
    torch.cuda.synchronize()
    return eng, p, tgt, idx


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("scen,N,S,graph,k,conv", TD_SHAPES)
def test_td_gamma_against_the_oracle(sw, golden_weights, scen, N, S, graph, k, conv, gamma):
    """swarm_td_grad at gamma other than 0.99: the loss and the gradient against the oracle's autograd
    at that gamma, with test_td_update_parity's bounds.  Guard: the oracle's gradient at this gamma and
    at 0.99 differ by more than 10x the per-element bound on more than 1 % of the elements.  At
    gamma = 0 the target network does not enter: two target weight sets give the same bits."""
    B = 16
    eng, p, tgt, idx = _td_case(sw, golden_weights, scen, N, S, graph, k, conv, gamma)
    slot, env = (idx // B).long(), (idx % B).long()
    s, s1 = eng.rep_s.cpu()[slot, env], eng.rep_s1.cpu()[slot, env]
    a, r = eng.rep_a.cpu()[slot, env].long(), eng.rep_r.cpu()[slot, env]
    edge_fn = None
    if graph == "knn":
        edge_fn = lambda ss: torch.cat([O.knn_edge_index(ss[g, :, :2], k) + g * N for g in range(ss.shape[0])], dim=1)  # noqa: E731
    loss32, g32s, _, g64 = oracle_grad_orders(p, tgt, s, a, r, s1, conv=conv, seed=S, edge_fn=edge_fn, gamma=gamma)
    grad = eng.grad.cpu()
    name = f"gamma={gamma} {scen} N={N} S={S} {graph} {conv}"
    assert_close_ulp(grad[NP].item() / (S * N), loss32, LOSS_ULP, f"{name} TD loss", scale=1.0, rel_floor=1e-5)
    _grad_bound_check(name, grad[:NP], g32s, g64)
    # guard: ignoring gamma (0.99 instead) moves the gradient by more than 10x the per-element bound
    ei = None if edge_fn is None else edge_fn(s)
    ein = None if edge_fn is None else edge_fn(s1)
    g64d = O.td_loss_grad(p, tgt, s, a, r, s1, 0.99, ei, ein, conv, dtype=torch.float64)[1]
    moved, o = [], 0
    for _, shape in O.PARAM_ORDER:
        n = int(np.prod(shape))
        b = g64[o:o + n]
        noise = torch.stack([(c[o:o + n].double() - b).abs() for c in g32s]).max(dim=0).values
        elem_bound = 1e-4 * b.abs() + 2e-6 * float(b.abs().max()) + 4.0 * noise
        moved.append((g64d[o:o + n] - b).abs() > 10.0 * elem_bound)
        o += n
    frac = float(torch.cat(moved).double().mean())
    record(f"{name}: guard, fraction of gradient elements moved by > 10x the bound vs gamma = 0.99", {"fraction": frac})
    assert frac > 0.01, (name, frac)
    if gamma == 0.0:
        eng2, _, _, _ = _td_case(sw, golden_weights, scen, N, S, graph, k, conv, gamma, tgt_seed=7)
        assert not torch.equal(eng2.target, eng.target)
        assert torch.equal(eng2.grad[:NP + 1], eng.grad[:NP + 1]), "r + 0 * max Q' is r: the target weights do not enter"


# ------------------------------------------------------------------ a mid-run change
NEW_VALUES = dict(lr=3e-4, gamma=0.5, betas=(0.5, 0.9), adam_eps=1e-3, max_norm=0.05, update_target_every=2)


@pytest.mark.parametrize("field", list(NEW_VALUES))
def test_three_paths_agree_through_a_mid_run_set_hp(sw, golden_weights, field):
    """train_tick, train_tick3 and train_tick_unfused from one seed: 4 ticks, set_hp(field), 5 more
    ticks, flush; weights, m, v, target, state and ctrl's optimizer words bit-equal.

    An optimizer step computes with the hyper-parameters of the launch that applies it.  The fused
    paths apply tick t's step in tick t + 1's launch, the unfused path in tick t's own
    swarm_adam_step, so "the same change" is set_hp before the launch that applies tick 3's step: on
    the fused engines between ticks 3 and 4, on the unfused engine between tick 3's TD launches
    (which take the old gamma on every path) and its swarm_adam_step.  Until adam_kernel rewrote
    ctrl's 1 - beta words after its step this failed for betas on the unfused path."""
    from swarm_amd.engine import HP_FIELDS
    assert set(NEW_VALUES) == set(HP_FIELDS)
    p = _params(golden_weights, "go_to", 4)
    kw = dict(seed=21, params=p, batch=24, eps=0.25, update_target_every=3, replay_capacity=4 * 16)
    engs = [sw.SwarmEngine("GoTo", 5, 16, **kw) for _ in range(3)]
    fused, tick3, unfused = engs
    assert fused.fused
    for e in engs:
        e.reset(0)
    change = {field: NEW_VALUES[field]}
    for t in range(9):
        if t == 4:
            fused.set_hp(**change)
            tick3.set_hp(**change)
        fused.train_tick()
        tick3.train_tick3()
        if t == 3:   # train_tick_unfused, with the change in front of its optimizer step
            unfused.act(push=True, full_out=False)
            unfused.flush()
            unfused.td_grad()
            unfused.allreduce_grad()
            unfused.set_hp(**change)
            unfused.adam()
        else:
            unfused.train_tick_unfused()
    for e in engs:
        e.flush()
    torch.cuda.synchronize()
    assert fused.handoff_errors() == 0
    assert fused.read_ctrl()["adam_step"] == 8
    for other, what in ((tick3, "3-launch tick"), (unfused, "unfused")):
        for k in ("params", "adam_m", "adam_v", "target", "state"):
            assert torch.equal(getattr(fused, k), getattr(other, k)), (field, what, k)
        assert torch.equal(fused.ctrl.cpu()[OPT_WORDS], other.ctrl.cpu()[OPT_WORDS]), (field, what, "ctrl")


@pytest.mark.parametrize("field", ["lr", "betas", "adam_eps", "max_norm"])
def test_transition_step_against_its_restatement(sw, p_init, field):
    """set_hp between optimizer steps 3 and 4 (swarm_adam_step, injected gradients).  Steps 1-3 are
    torch's with the old values.  Step 4, the first launched with the new values, takes the step
    size (old lr, old beta1's bias correction), bias correction 2 and 1 - beta from the control block
    as the launch before it left them, and eps, max_norm and v's decay beta2 from its own launch; from
    step 5 on every value is the new one, with bias corrections 1 - the product of the betas in
    force at each step (by design; torch's beta**step only while the betas never change):
    tests/hp_cases.py CtrlModel.  Each step against that restatement in float64 from the GPU's own
    p, m, v, within the bounds of the optimizer cases; steps 1-3 against torch itself too."""
    old = dict(H.DEFAULTS)
    new = dict(old, **{field: NEW_VALUES[field]})
    eng = _tiny(sw, p_init, old)
    model = H.CtrlModel(old)
    seen, noise = [], dict.fromkeys(H.PROJECT_ULP, 0.0)
    for s in range(H.N_STEPS):
        hp = old if s < 3 else new
        if s == 3:
            eng.set_hp(**{field: NEW_VALUES[field]})
        g = H.synthetic_grad(f"transition {field}", s, kind="std")
        p0, m0, v0 = _pmv(eng)
        _inject(eng, g)
        eng.adam()
        p1, m1, v1 = _pmv(eng)
        sc = model.step(hp)
        r64 = H.adam_ref64(p0, g, m0, v0, sc, hp["adam_eps"], hp["max_norm"])
        sc_ = H.scales(p0, m0, v0, r64, sc, min(old["lr"], new["lr"]))
        n = H.ulp_errors(H.adam_np32(p0, g, m0, v0, sc, hp["adam_eps"], hp["max_norm"]), r64, sc_)
        noise = {k: max(noise[k], n[k]) for k in noise}
        got = dict(p=p1, m=m1, v=v1, norm=eng.read_ctrl()["grad_norm"])
        seen.append(H.ulp_errors(got, r64, sc_))
        if s < 3:
            _adam_check(f"hp transition {field} step {s}", p1, m1, v1, p0, g, m0, v0, s, norm_gpu=got["norm"])
        if s == 3:   # the restatement is a mixture: a step with either set alone is > 10x the bound away
            for alt in (old, new):
                r_alt = H.adam_ref64(p0, g, m0, v0, H.adam_scalars(alt["lr"], *alt["betas"], s), alt["adam_eps"],
                                     alt["max_norm"])
                q = {"lr": "p", "betas": "v", "adam_eps": "p", "max_norm": "m"}[field]
                frac = H.guard_fraction(r64, r_alt, sc_, H.PROJECT_ULP[q], q)
                which = "old" if alt is old else "new"
                record(f"hp transition {field}: step 4 vs a step with the {which} values alone, {q}", {"fraction": frac})
                expect_same = (field in ("adam_eps", "max_norm") and alt is new) or (field == "lr" and alt is old)
                assert (frac == 0.0) if expect_same else (frac > 0.01), (field, which, frac)
    bound = H.bounds_from_noise(noise)
    record(f"hp transition {field}: asserted bounds (ulp)", bound)
    for s, err in enumerate(seen):
        record(f"hp transition {field} step {s}: gpu vs the float64 restatement (ulp)", err)
        for k in err:
            assert err[k] <= bound[k], (field, s, k, err[k], bound[k])
