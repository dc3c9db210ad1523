"""GPU tests of the three-layer GAT's learner on the unfused device path: swarm_gat3_td_grad and
swarm_gat3_adam_step through the C ABI, ``SwarmGat3Engine`` and ``DQNTrainer(net="gat3")``.

Gradient reference: the float64 evaluation of train_gcn_dqn.py:113-124 with the oracle's
``gat3_q_forward_dense``, its multiplicities built by ``graph_multiplicity`` from s for the online
net and from s' for the target net, and ``MSELoss``.  Bar: tests/test_q_backward.py's GRAD_TOL, the
project's gradient bar, max|g - g64| / max(max|g64|, 1e-3) < 2e-5; each parity case first asserts
that the oracle's own fp32 evaluation is below 2.8e-6 in that metric (tests/test_gat3_backward.py).
The optimizer is compared with torch's ``clip_grad_norm_`` + ``Adam(foreach=False)`` fed the GPU's own
gradient, so the gradient's rounding does not enter: 2e-6 on the parameters after a step (the
project's bar for a step), 5e-6 after three (tests/test_gpu_parity.py's multi-step bar)."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import swarm_oracle as O
from tests.conftest import record

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-5            # tests/test_q_backward.py GRAD_TOL
ORACLE_FP32_MAX = 2.8e-6   # tests/test_gat3_backward.py: the oracle's own fp32 evaluation
LOSS_TOL = 1e-5            # the floor of the existing TD test
GRAPH = {"complete": 0, "knn": 1, "radius": 3}
OGRAPH = {"complete": O.GRAPH_COMPLETE, "knn": O.GRAPH_KNN, "radius": O.GRAPH_RADIUS}
RADIUS = 0.5
GAMMA = 0.99
NP3 = O.GAT3_N_PARAMS
B_RING = 16

# (N, S, graph, k)
CASES = [
    (2, 9, "complete", 0),
    (5, 7, "complete", 0),          # a partly filled last block
    (8, 32, "complete", 0),
    (8, 260, "complete", 0),        # 65 slabs: the reduce's groups take two each
    (8, 32, "radius", 0),
    (8, 32, "knn", 5),
    (12, 24, "knn", 5), (16, 4, "knn", 5),                                                    # 16 slots
    (9, 5, "complete", 0),
    (20, 6, "knn", 10), (29, 3, "complete", 0), (32, 2, "knn", 10), (17, 3, "radius", 0),     # 32 slots
]
PAIRS = [(4, 8), (2, 4), (8, 2)]   # (online, target) Flocking checkpoint seeds


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _weights(golden_weights, seed):
    return torch.tensor(golden_weights["flocking_gat3"][seed])


@functools.lru_cache(maxsize=None)
def _case_inputs(N, S):
    g = torch.Generator().manual_seed(1000 * N + S)
    s = torch.randn(S, N, 4, generator=g) * 0.4
    s1 = s + torch.randn(S, N, 4, generator=g) * 0.05
    a = torch.randint(0, 9, (S, N), generator=g)
    r = torch.randn(S, N, generator=g)
    cap = max(4, -(-S // B_RING))
    idx = torch.randperm(cap * B_RING, generator=g)[:S].to(torch.int32)
    return s, s1, a, r, cap, idx


def _flat_grad(P):
    return torch.cat([(P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).reshape(-1)
                      for k, _ in O.GAT3_PARAM_ORDER])


def _oracle_td(p, tgt, s, a, r, s1, graph, k, dtype, gamma=GAMMA):
    """train_gcn_dqn.py:113-124 with the three-layer network: (flat gradient, loss)."""
    S, N, _ = s.shape
    P = {kk: v.to(dtype).clone().requires_grad_(True) for kk, v in O.gat3_unflatten(p).items()}
    T = {kk: v.to(dtype) for kk, v in O.gat3_unflatten(tgt).items()}
    mult = O.graph_multiplicity(s[..., :2], OGRAPH[graph], k, RADIUS).to(dtype)
    mult1 = O.graph_multiplicity(s1[..., :2], OGRAPH[graph], k, RADIUS).to(dtype)
    x = O.node_features(s[..., :2], s[..., 2:4]).to(dtype)
    xn = O.node_features(s1[..., :2], s1[..., 2:4]).to(dtype)
    values = O.gat3_q_forward_dense(P, x, mult).reshape(S * N, -1).gather(1, a.reshape(-1, 1).long())
    with torch.no_grad():
        next_values = O.gat3_q_forward_dense(T, xn, mult1).reshape(S * N, -1).max(dim=1)[0]
    target = r.reshape(-1).to(dtype) + gamma * next_values
    loss = torch.nn.MSELoss()(values, target.unsqueeze(1))
    loss.backward()
    return _flat_grad(P), float(loss.detach())


def _metric(g, g64):
    return ((g.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-3)).item()


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.contiguous().numpy().view(np.uint8), b.contiguous().numpy().view(np.uint8))


class _Learner:
    """The two entry points through the C ABI on buffers of its own: a ring of ``cap`` slots of B
    envs, 416-float params / target / m / v / grad, a control block from swarm_ctrl_init."""

    def __init__(self, N, B, cap, S, graph, k, p, tgt, seed=0, every=200, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8,
                 max_norm=1.0):
        import swarm_amd._lib as L
        self.L, self.lib = L, L.load()
        self.N, self.B, self.cap, self.S = N, B, cap, S
        self.cfg = L.SwarmConfig(B, N, O.SCENARIO_FLOCK, GRAPH[graph], k, L.CONV_GAT, 0, 0, seed,
                                 RADIUS if graph == "radius" else 0.0, L.NET_GAT3)
        # the double fields as SwarmEngine sets them
        self.hp = L.SwarmAdamCfg(lr, betas[0], betas[1], adam_eps, max_norm, GAMMA, S, every, 1, 0, float(lr),
                                 float(betas[0]), float(betas[1]))
        dev = dict(device="cuda", dtype=torch.float32)
        n_ws = self.lib.swarm_td_workspace_floats(ctypes.byref(self.cfg), S)
        assert n_ws > 0
        self.ws = torch.empty(n_ws, **dev)
        self.grad = torch.empty(L.GAT3_GRAD_FLOATS, **dev)
        self.rows = torch.zeros(4, L.GAT3_GRAD_FLOATS, **dev)   # params, target, m, v
        self.rows[:, NP3:] = 7.0                                 # floats 409..415: left as they are
        self.rows[0, :NP3] = p.cuda()
        self.rows[1, :NP3] = tgt.cuda()
        self.params, self.target, self.m, self.v = self.rows[0], self.rows[1], self.rows[2], self.rows[3]
        self.rep_s = torch.zeros(cap, B, N, 4, **dev)
        self.rep_s1 = torch.zeros(cap, B, N, 4, **dev)
        self.rep_r = torch.zeros(cap, B, N, **dev)
        self.rep_a = torch.zeros(cap, B, N, dtype=torch.uint8, device="cuda")
        self.replay = L.SwarmReplay(L.ptr(self.rep_s), L.ptr(self.rep_s1), L.ptr(self.rep_r), L.ptr(self.rep_a), cap, 0)
        self.ctrl = torch.zeros(L.CTRL_WORDS, dtype=torch.int32, device="cuda")
        assert self.lib.swarm_ctrl_init(ctypes.byref(self.hp), 0.0, L.ptr(self.ctrl), L.stream_ptr()) == 0
        self.sample_in = None
        self.sample_out = None
        self.poison()

    def fill(self, idx, s, s1, a, r):
        """transition i of the batch into the ring row sample_in[i] names"""
        slot, env = (idx // self.B).long(), (idx % self.B).long()
        self.rep_s[slot, env] = s.cuda()
        self.rep_s1[slot, env] = s1.cuda()
        self.rep_r[slot, env] = r.cuda()
        self.rep_a[slot, env] = a.to(torch.uint8).cuda()
        self.sample_in = idx.cuda()

    def set_ctrl(self, tick=None, filled=None):
        if tick is not None:
            self.ctrl[self.L.CTRL["tick"]] = tick
        if filled is not None:
            self.ctrl[self.L.CTRL["filled_slots"]] = filled

    def poison(self):
        self.ws.fill_(float("nan"))
        self.grad.fill_(float("nan"))

    def td(self):
        L = self.L
        rc = self.lib.swarm_gat3_td_grad(ctypes.byref(self.cfg), ctypes.byref(self.hp), L.ptr(self.params),
                                         L.ptr(self.target), ctypes.byref(self.replay), L.ptr(self.ctrl),
                                         L.ptr(self.sample_in), L.ptr(self.sample_out), L.ptr(self.ws), L.ptr(self.grad),
                                         L.stream_ptr())
        assert rc == 0, rc

    def adam(self):
        L = self.L
        rc = self.lib.swarm_gat3_adam_step(ctypes.byref(self.cfg), ctypes.byref(self.hp), L.ptr(self.params),
                                           L.ptr(self.target), L.ptr(self.m), L.ptr(self.v), L.ptr(self.grad), self.cap,
                                           L.ptr(self.ctrl), L.stream_ptr())
        assert rc == 0, rc

    def run_td(self):
        self.poison()
        self.td()
        torch.cuda.synchronize()
        return self.grad.cpu()

    def read_ctrl(self):
        from swarm_amd.engine import decode_ctrl
        return decode_ctrl(self.ctrl.cpu())


def _learner_for_case(N, S, graph, k, p, tgt, **kw):
    s, s1, a, r, cap, idx = _case_inputs(N, S)
    lr = _Learner(N, B_RING, cap, S, graph, k, p, tgt, **kw)
    lr.fill(idx, s, s1, a, r)
    lr.set_ctrl(filled=cap)
    return lr


# ------------------------------------------------------------------ 1. TD gradient parity through the C ABI
@pytest.mark.parametrize("pair", PAIRS, ids=lambda pr: f"w{pr[0]}t{pr[1]}")
@pytest.mark.parametrize("N,S,graph,k", CASES)
def test_gat3_td_grad_parity(sw, golden_weights, N, S, graph, k, pair):
    """Figures of the run recorded in profiles/gat3_td_parity_errors.json."""
    p, tgt = _weights(golden_weights, pair[0]), _weights(golden_weights, pair[1])
    s, s1, a, r, cap, idx = _case_inputs(N, S)
    g64, loss64 = _oracle_td(p, tgt, s, a, r, s1, graph, k, torch.float64)
    g32, loss32 = _oracle_td(p, tgt, s, a, r, s1, graph, k, torch.float32)
    fp32_err = _metric(g32, g64) if torch.isfinite(g32).all() else float("nan")
    assert fp32_err < ORACLE_FP32_MAX, f"precondition: the oracle's own fp32 evaluation is at {fp32_err:.3e}"
    out = _learner_for_case(N, S, graph, k, p, tgt).run_td()
    assert out.shape == (416,)
    assert torch.isfinite(out).all(), "an unwritten slab column (NaN workspace) or a non-finite sum"
    g = out[:NP3]
    err = _metric(g, g64)
    loss = float(out[NP3]) / (S * N)
    loss_err = abs(loss - loss64) / abs(loss64)
    zero = g64 == 0
    rec = record(f"gat3_td_grad N={N} S={S} {graph} k={k} weights={pair[0]} target={pair[1]}",
                 dict(n=NP3, max_abs=float((g.double() - g64).abs().max()), max_rel=err),
                 oracle_fp32=fp32_err, tol_rel=GRAD_TOL, loss_rel=loss_err, loss_oracle_fp32=abs(loss32 - loss64) / abs(loss64),
                 exact_zeros=int(zero.sum()))
    print(rec)
    assert err < GRAD_TOL, f"gradient: {err:.3e} (oracle fp32 {fp32_err:.3e})"
    assert loss_err < LOSS_TOL, f"loss: {loss} vs {loss64} ({loss_err:.3e})"
    assert (out[NP3 + 1:] == 0).all(), "columns 410..415"
    assert (g[zero] == 0).all(), "a parameter whose float64 gradient is exactly 0 (dead relu units)"


# ------------------------------------------------------------------ 2. sampling
def test_gat3_td_sampling_matches_oracle_and_is_distinct(sw, golden_weights):
    B, N, S = 32, 4, 100
    p = _weights(golden_weights, 4)
    lr = _Learner(N, B, 10, S, "complete", 0, p, p, seed=123)
    lr.set_ctrl(tick=17, filled=6)     # filled slots -> 7 valid slots after this tick's push
    lr.sample_out = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    lr.run_td()
    got = lr.sample_out.cpu().tolist()
    n = 7 * B
    assert len(set(got)) == S and all(0 <= x < n for x in got)
    assert got == [O.sample_index(i, n, seed=123, rnd=17) for i in range(S)]   # env_offset 0 -> key unchanged


# ------------------------------------------------------------------ 3. skip
def test_gat3_td_skips_until_the_ring_holds_a_batch(sw, golden_weights):
    p, tgt = _weights(golden_weights, 4), _weights(golden_weights, 8)
    lr = _Learner(8, 16, 4, 33, "complete", 0, p, tgt)   # 1 valid slot = 16 graphs < 33
    lr.sample_out = torch.full((33,), -1, dtype=torch.int32, device="cuda")
    out = lr.run_td()
    assert (out == 0).all() and out.shape == (416,)
    ws = lr.ws.cpu()
    n_slabs = -(-33 // 4)
    assert not torch.isnan(ws[: n_slabs * 416]).any() and (ws[: n_slabs * 416] == 0).all()
    assert (lr.sample_out.cpu() == -1).all()
    rows0 = lr.rows.cpu()
    lr.adam()
    torch.cuda.synchronize()
    assert _bits(lr.rows.cpu(), rows0)
    c = lr.read_ctrl()
    assert c["adam_step"] == 0 and c["loss"] == 0 and c["grad_norm"] == 0 and c["trained"] == 0
    assert c["tick"] == 1 and c["filled_slots"] == 1 and c["write_slot"] == 1


# ------------------------------------------------------------------ 4. the optimizer, fed the GPU's own gradient
def _torch_step(pr, g, opt, max_norm):
    pr.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([pr], max_norm)
    opt.step()


@pytest.mark.parametrize("hp", [{}, dict(lr=3e-4, betas=(0.8, 0.99), adam_eps=1e-6, max_norm=0.5)],
                         ids=["defaults", "lr3e-4_b0.8_0.99_eps1e-6_clip0.5"])
def test_gat3_adam_step_matches_torch(sw, golden_weights, hp):
    p, tgt = _weights(golden_weights, 4), _weights(golden_weights, 8)
    lr = _learner_for_case(8, 32, "complete", 0, p, tgt, **hp)
    g = lr.run_td()[:NP3].clone()
    kw = dict(dict(lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8, max_norm=1.0), **hp)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=kw["lr"], betas=kw["betas"], eps=kw["adam_eps"], foreach=False)
    _torch_step(pr, g, opt, kw["max_norm"])
    lr.adam()
    torch.cuda.synchronize()
    rows = lr.rows.cpu()
    ref_norm = float(g.double().norm())
    c = lr.read_ctrl()
    m_ref, v_ref = opt.state[pr]["exp_avg"], opt.state[pr]["exp_avg_sq"]
    errs = dict(params=float((rows[0, :NP3] - pr.detach()).abs().max()),
                grad_norm=abs(c["grad_norm"] - ref_norm),
                m=float((rows[2, :NP3] - m_ref).abs().max() / m_ref.abs().max()),
                v=float((rows[3, :NP3] - v_ref).abs().max() / v_ref.abs().max()))
    print(record(f"gat3_adam_step vs torch {sorted(hp.items())}", dict(n=NP3, max_abs=errs["params"], max_rel=errs["m"]),
                 **errs, ref_norm=ref_norm))
    assert errs["params"] < 2e-6
    assert errs["grad_norm"] <= 1e-5 * max(1.0, ref_norm)
    assert errs["m"] < 1e-5 and errs["v"] < 1e-5
    assert c["adam_step"] == 1 and c["trained"] == 0 and c["tick"] == 1
    assert not torch.equal(rows[0, :NP3], p)
    assert _bits(rows[1, :NP3], tgt), "no target sync at tick 0 of 200"
    assert (rows[:, NP3:] == 7.0).all(), "floats 409..415 are left as they are"
    loss = float(lr.grad.cpu()[NP3]) / (32 * 8)
    assert c["loss"] == pytest.approx(loss, rel=1e-6) and loss > 0


def test_gat3_multi_step_adam_parity(sw, golden_weights):
    """Three consecutive updates (bias corrections, state carry-over, target sync every 2) against
    torch's optimizer, each step fed the GPU's gradient of that step."""
    N, S, cap = 8, 24, 4
    p, tgt = _weights(golden_weights, 4), _weights(golden_weights, 8)
    s, s1, a, r, _, _ = _case_inputs(N, 32)
    lr = _Learner(N, B_RING, cap, S, "complete", 0, p, tgt, every=2)
    ring = torch.randperm(cap * B_RING, generator=torch.Generator().manual_seed(99))[:32].to(torch.int32)
    lr.fill(ring, s, s1, a, r)
    pr = p.clone().requires_grad_(True)
    rt = tgt.clone()
    opt = torch.optim.Adam([pr], lr=1e-3, foreach=False)
    for step in range(3):
        lr.sample_in = ring[torch.randperm(32, generator=torch.Generator().manual_seed(step))[:S]].cuda()
        lr.set_ctrl(tick=step, filled=cap)   # (tick + 1) % 2 == 0 syncs the target after step 1
        g = lr.run_td()[:NP3].clone()
        assert torch.isfinite(g).all() and g.any()
        target_before = lr.target.cpu()
        lr.adam()
        torch.cuda.synchronize()
        _torch_step(pr, g, opt, 1.0)
        if (step + 1) % 2 == 0:
            rt = pr.detach().clone()
            assert _bits(lr.target.cpu()[:NP3], lr.params.cpu()[:NP3]), "the sync step copies the new weights"
        else:
            assert _bits(lr.target.cpu(), target_before), "the target is untouched between syncs"
        assert lr.read_ctrl()["adam_step"] == step + 1
    assert (lr.params.cpu()[:NP3] - pr.detach()).abs().max().item() < 5e-6
    assert (lr.target.cpu()[:NP3] - rt).abs().max().item() < 5e-6


# ------------------------------------------------------------------ 5. determinism and capture
def test_gat3_td_grad_is_deterministic(sw, golden_weights):
    lr = _learner_for_case(8, 33, "knn", 5, _weights(golden_weights, 4), _weights(golden_weights, 8))
    a = lr.run_td()
    ws_a = lr.ws.cpu()
    b = lr.run_td()
    assert torch.isfinite(a).all() and a[:NP3].any()
    assert _bits(a, b) and _bits(ws_a, lr.ws.cpu())


def test_gat3_td_and_adam_are_capturable(sw, golden_weights):
    """td_grad + adam_step (three launches in one chain) captured on a side stream and replayed:
    the eager run's bits."""
    from swarm_amd.engine import capture_ticks
    lr = _learner_for_case(8, 33, "knn", 5, _weights(golden_weights, 4), _weights(golden_weights, 8))
    rows0, ctrl0 = lr.rows.clone(), lr.ctrl.clone()

    def step():
        lr.td()
        lr.adam()

    lr.poison()
    step()
    torch.cuda.synchronize()
    eager = (lr.grad.cpu(), lr.rows.cpu(), lr.ctrl.cpu())
    assert torch.isfinite(eager[0]).all() and lr.read_ctrl()["adam_step"] == 1
    graph = capture_ticks(torch.device("cuda"), 1, step)
    for _ in range(2):
        lr.rows.copy_(rows0)
        lr.ctrl.copy_(ctrl0)
        lr.poison()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(lr.grad.cpu(), eager[0]) and _bits(lr.rows.cpu(), eager[1]) and _bits(lr.ctrl.cpu(), eager[2])


# ------------------------------------------------------------------ 6. the engine
def test_gat3_engine_trains(sw, golden_weights):
    p = _weights(golden_weights, 4)
    kw = dict(seed=3, params=p, batch=16, replay_capacity=64)
    eng = sw.SwarmGat3Engine("Flocking", 6, 8, **kw)
    assert eng.net == "gat3" and not eng.fused and eng.capacity == 8
    eng.reset(0)
    eng.train_tick()
    c = eng.read_ctrl()
    assert c["adam_step"] == 0 and c["tick"] == 1 and torch.equal(eng.params.cpu(), p)   # 8 graphs < 16
    before = eng.state.clone()
    tgt_before = eng.target.cpu()
    p_before = eng.params.cpu()
    eng.train_tick()
    c = eng.read_ctrl()
    assert c["adam_step"] == 1 and c["loss"] > 0 and c["trained"] == 0 and c["tick"] == 2
    assert torch.equal(eng.rep_s[1], before) and torch.equal(eng.rep_s1[1], eng.state)
    assert not torch.equal(eng.params.cpu(), p_before)
    # tick 1's gradient from the ring's contents at engine.samples
    idx = eng.samples.cpu().long()
    assert len(set(idx.tolist())) == 16 and int(idx.max()) < 16
    slot, env = idx // 8, idx % 8
    s, s1 = eng.rep_s.cpu()[slot, env], eng.rep_s1.cpu()[slot, env]
    a, r = eng.rep_a.cpu()[slot, env].long(), eng.rep_r.cpu()[slot, env]
    g64, loss64 = _oracle_td(p_before, tgt_before, s, a, r, s1, "complete", 0, torch.float64)
    g = eng.grad.cpu()[:NP3]
    err = _metric(g, g64)
    print(record("gat3 engine tick 1 TD grad", dict(n=NP3, max_abs=float((g.double() - g64).abs().max()), max_rel=err),
                 tol_rel=GRAD_TOL))
    assert err < GRAD_TOL, err
    assert abs(c["loss"] - loss64) / loss64 < LOSS_TOL
    eng.train_tick()
    eng.train_tick()
    torch.cuda.synchronize()
    # the same 4 ticks from a captured graph
    cap = sw.SwarmGat3Engine("Flocking", 6, 8, **kw)
    cap.reset(0)
    graph = cap.capture(4)
    graph.replay()
    torch.cuda.synchronize()
    assert eng.read_ctrl()["adam_step"] == 3
    for name in ("params", "target", "adam_m", "adam_v", "ctrl", "state"):
        assert torch.equal(getattr(eng, name), getattr(cap, name)), name
    with pytest.raises(ValueError, match="unfused"):
        eng.train_tick3()
    with pytest.raises(ValueError):
        sw.SwarmGat3Engine("Flocking", 6, 8, world_size=2, **kw)
    with pytest.raises(ValueError, match="conv"):
        sw.SwarmGat3Engine("Flocking", 6, 8, conv="gcn", **kw)
    # a batch larger than the one the slabs and ``samples`` were sized for is refused before any launch
    eng.hp.batch = 17
    with pytest.raises(ValueError, match="batch"):
        eng.td_update()
    eng.hp.batch = 16
    with pytest.raises(ValueError, match="sample_out"):
        eng.td_grad(sample_out=eng.samples[:8])
    assert eng.read_ctrl()["adam_step"] == 3
    with pytest.raises(ValueError):
        sw.SwarmEngine("Flocking", 6, 8, net="gat3", learn=True, **kw)


def test_gat3_engine_fresh_init(sw):
    from swarm_amd.engine import unflatten_params
    eng = sw.SwarmGat3Engine("Flocking", 6, 8, seed=3, params=None, batch=16, replay_capacity=64)
    flat = eng.params.cpu()
    assert flat.shape == (409,) and torch.isfinite(flat).all() and torch.equal(flat, eng.target.cpu())
    sd = unflatten_params(flat, "gat3")
    assert all(not sd[f"conv{i}.bias"].any() and sd[f"conv{i}.lin.weight"].any() for i in (1, 2, 3))
    assert list(eng.state_dict()) == [k for k, _ in O.GAT3_PARAM_ORDER]


# ------------------------------------------------------------------ 7. the trainer
def test_gat3_trainer(sw, tmp_path):
    seed = 1
    env = sw.make_env(scenario=sw.FlockingScenario(), num_envs=4, continuous_actions=False, wrapper=None, max_steps=6,
                      dict_spaces=True, n_agents=4, seed=seed)
    sw.set_seed(seed)
    models, stats = str(tmp_path / "models"), str(tmp_path / "stats")
    tr = sw.DQNTrainer(env, seed, models, stats, "Flocking", net="gat3", batch_size=8, replay_capacity=1000)
    assert isinstance(tr.engine, sw.SwarmGat3Engine) and isinstance(tr.model, sw.GAT3)
    init = {k: v.clone() for k, v in tr.model.state_dict().items()}
    config = {"epsilon": 0.99, "epsilon_decay": 0.01, "min_epsilon": 0.05, "episodes": 2, "eval_every": 1, "eval_envs": 3}
    with pytest.raises(ValueError, match="pbt_every"):
        tr.train_model(dict(config, pbt_every=1))
    tr.train_model(config)   # the second episode is captured and replayed
    sd = torch.load(os.path.join(models, f"experiment_Flocking-seed_{seed}.pth"), weights_only=True)
    assert list(sd) == [k for k, _ in O.GAT3_PARAM_ORDER]
    m = sw.GCN.from_state_dict(sd)
    assert isinstance(m, sw.GAT3)
    assert os.path.exists(os.path.join(stats, f"experiment_Flocking-seed_{seed}.csv"))
    assert os.path.exists(os.path.join(stats, f"experiment_Flocking-seed_{seed}-eval.csv"))
    assert len(tr.eval_rows) == 2 and all(math.isfinite(x) for row in tr.eval_rows for x in row)
    assert any(not torch.equal(sd[k], init[k]) for k in sd)
    assert all(torch.isfinite(v).all() for v in sd.values())
    # 'Loss' is logged by the ticks that ran an update: every tick but the first (4 graphs < 8)
    assert [t for t, _ in tr.writer.scalars["Loss"]] == list(range(2, 13))
    assert tr.engine.read_ctrl()["adam_step"] == 11
    with pytest.raises(ValueError):
        sw.PopulationTrainer([tr])
