"""GPU parity of swarm_gat3_q_backward (the backward of the three-layer GAT for a caller's dL/dQ) and
of the ``GAT3(autograd=True)`` binding, against the oracle's torch autograd through
``gat3_q_forward_dense`` / ``gat3_q_forward_edges`` evaluated in float64 from the same fp32 inputs.

Bar: tests/test_q_backward.py's GRAD_TOL, the project's gradient bar, taken over:
max|g_gpu - g64| / max(max|g64|, 1e-3) < 2e-5.  Weights: the Flocking checkpoints of seeds 2, 4 and
8, on which the oracle's own fp32 autograd stays below 2.8e-6 in that metric on every case here (each
parity case asserts it first); on seeds 5 and 9 the oracle's fp32 reaches 1.1e-5, and seed 9's fp32
backward is NaN on graphs with an in-edge-less node: a property of the reference, so they are left out.
Inputs follow tests/test_q_backward.py::_inputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import swarm_oracle as O
from tests.conftest import record

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-5          # tests/test_q_backward.py GRAD_TOL
ORACLE_FP32_MAX = 2.8e-6   # the level tests/test_q_backward.py documents for the oracle's fp32 evaluation
GRAPH = {"complete": 0, "knn": 1, "dense": 2, "radius": 3}
RADIUS = 0.5
NP3 = O.GAT3_N_PARAMS

# (N, B, graph, k, weights seed, holes)
CASES = [
    (1, 3, "complete", 0, 4, False), (2, 9, "complete", 0, 4, False),
    (5, 7, "complete", 0, 2, False),        # last block partly filled
    (8, 33, "complete", 0, 4, False),
    (8, 260, "complete", 0, 8, False),      # 65 slabs: the reduce's groups take two slabs each
    (9, 5, "complete", 0, 2, False), (16, 4, "knn", 5, 4, False),   # 16-slot graphs
    (17, 3, "dense", 0, 8, False), (29, 2, "complete", 0, 2, False), (32, 2, "knn", 10, 4, False),   # 32-slot graphs
    (8, 6, "radius", 0, 8, False),          # 5 nodes without an in-edge
    (6, 4, "dense", 0, 4, False),           # multiplicities up to 3
    (6, 3, "dense", 0, 2, True),            # a node with no in-edge and a graph with no edge
]


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _weights(golden_weights, seed):
    return torch.tensor(golden_weights["flocking_gat3"][seed])


def _inputs(N, B, graph, holes=False):
    """tests/test_q_backward.py::_inputs: state, features, (dense) multiplicities, dL/dQ from one generator."""
    g = torch.Generator().manual_seed(100 * N + B)
    s = torch.randn(B, N, 4, generator=g) * 0.4
    x = O.node_features(s[..., :2], s[..., 2:4])
    if graph == "dense":
        mult = torch.randint(0, 4, (B, N, N), generator=g)
        if holes:
            mult[0, :, 2] = 0
            mult[1] = 0
    else:
        mult = None
    dq = torch.randn(B, N, 9, generator=g)
    return s, x, mult, dq


def _flat_grad(P):
    return torch.cat([(P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).reshape(-1)
                      for k, _ in O.GAT3_PARAM_ORDER])


def _oracle_grad(p, x, mult, dq, dtype=torch.float64):
    """d (q * dq).sum() / d params by the oracle's autograd on the dense multiplicity form."""
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in O.gat3_unflatten(p).items()}
    q = O.gat3_q_forward_dense(P, x.to(dtype), mult.to(dtype))
    (q * dq.to(dtype)).sum().backward()
    return _flat_grad(P)


@functools.lru_cache(maxsize=None)
def _case_inputs(N, B, graph, k, holes):
    s, x, mult, dq = _inputs(N, B, graph, holes)
    if graph != "dense":   # the multiplicities the kernel builds itself, for the oracle
        og = {"complete": O.GRAPH_COMPLETE, "knn": O.GRAPH_KNN, "radius": O.GRAPH_RADIUS}[graph]
        mult = O.graph_multiplicity(s[..., :2], og, k, RADIUS)
    return s, x, mult, dq


def _metric(g, g64):
    return ((g.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-3)).item()


class _Call:
    """One swarm_gat3_q_backward call through the C ABI on buffers of its own; workspace and grad
    are pre-filled with NaN before every run."""

    def __init__(self, N, B, graph, k, p, x, mult, dq):
        import swarm_amd._lib as L
        self.L, self.lib = L, L.load()
        self.cfg = L.SwarmConfig(B, N, O.SCENARIO_FLOCK if N >= 2 else O.SCENARIO_GOTO, GRAPH[graph], k, L.CONV_GAT,
                                 0, 0, 0, RADIUS if graph == "radius" else 0.0, L.NET_GAT3)
        n_ws = self.lib.swarm_td_workspace_floats(ctypes.byref(self.cfg), B)
        assert n_ws > 0
        dev = dict(device="cuda", dtype=torch.float32)
        self.ws = torch.empty(n_ws, **dev)
        self.grad = torch.empty(L.GAT3_GRAD_FLOATS, **dev)
        self.p = p.to(**dev).contiguous()
        self.x = x.reshape(B * N, 7).to(**dev).contiguous()
        self.dq = dq.reshape(B * N, 9).to(**dev).contiguous()
        self.mult = mult.to(torch.uint8).cuda().contiguous() if graph == "dense" else None
        self.poison()

    def poison(self):
        self.ws.fill_(float("nan"))
        self.grad.fill_(float("nan"))

    def launch(self):
        L = self.L
        rc = self.lib.swarm_gat3_q_backward(ctypes.byref(self.cfg), L.ptr(self.p), L.ptr(self.x), L.ptr(self.mult),
                                            L.ptr(self.dq), L.ptr(self.ws), L.ptr(self.grad), L.stream_ptr())
        assert rc == 0, rc

    def run(self):
        self.poison()
        self.launch()
        torch.cuda.synchronize()
        return self.grad.cpu()


def _bits(a, b):
    return np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


# ------------------------------------------------------------------ 1. parity through the C ABI
@pytest.mark.parametrize("N,B,graph,k,seed,holes", CASES)
def test_gat3_q_backward_parity(sw, golden_weights, N, B, graph, k, seed, holes):
    p = _weights(golden_weights, seed)
    s, x, mult, dq = _case_inputs(N, B, graph, k, holes)
    g64 = _oracle_grad(p, x, mult, dq)
    g32 = _oracle_grad(p, x, mult, dq, torch.float32)
    fp32_err = _metric(g32, g64) if torch.isfinite(g32).all() else float("nan")
    assert fp32_err < ORACLE_FP32_MAX, f"precondition: the oracle's own fp32 autograd is at {fp32_err:.3e}"
    out = _Call(N, B, graph, k, p, x, mult, dq).run()
    assert out.shape == (416,)
    assert torch.isfinite(out).all(), "an unwritten slab column (NaN workspace) or a non-finite sum"
    g = out[:NP3]
    err = _metric(g, g64)
    zero = g64 == 0
    rec = record(f"gat3_q_backward grad N={N} B={B} {graph} seed={seed}" + (" holes" if holes else ""),
                 dict(n=NP3, max_abs=float((g.double() - g64).abs().max()), max_rel=err),
                 oracle_fp32=fp32_err, tol_rel=GRAD_TOL, exact_zeros=int(zero.sum()))
    print(rec)
    assert err < GRAD_TOL, f"gradient: {err:.3e} (oracle fp32 {fp32_err:.3e})"
    assert (out[NP3:] == 0).all(), "columns 409..415"
    assert (g[zero] == 0).all(), "a parameter whose float64 gradient is exactly 0 (dead relu units)"


# ------------------------------------------------------------------ 2. determinism, 3. capture
def test_gat3_q_backward_is_deterministic(sw, golden_weights):
    s, x, mult, dq = _case_inputs(8, 33, "complete", 0, False)
    call = _Call(8, 33, "complete", 0, _weights(golden_weights, 4), x, mult, dq)
    a = call.run()
    ws_a = call.ws.cpu()
    b = call.run()
    assert torch.isfinite(a).all()
    assert _bits(a, b) and _bits(ws_a, call.ws.cpu())


def test_gat3_q_backward_is_capturable(sw, golden_weights):
    """Captured once on a side stream (two launches in one chain), replayed twice: the eager bits."""
    from swarm_amd.engine import capture_ticks
    s, x, mult, dq = _case_inputs(8, 33, "complete", 0, False)
    call = _Call(8, 33, "complete", 0, _weights(golden_weights, 4), x, mult, dq)
    eager = call.run()
    assert torch.isfinite(eager).all()
    graph = capture_ticks(torch.device("cuda"), 1, call.launch)
    for _ in range(2):
        call.poison()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(call.grad.cpu(), eager)


# ------------------------------------------------------------------ 4. the reference's training step
def _obs(s):
    """[B, N, 6] observations (pos, vel, goal) of states [B, N, 4]."""
    return O.node_features(s[..., :2], s[..., 2:4])[..., :6]


def _model(sw, flat, autograd=False):
    m = sw.GAT3(autograd=autograd)
    m.load_state_dict(O.gat3_unflatten(flat))
    return m


def _named_grad(model):
    named = dict(model.named_parameters())
    return torch.cat([named[k].grad.reshape(-1).cpu() for k, _ in O.GAT3_PARAM_ORDER])


def _oracle_td_grad(p, tgt, s, actions, rewards, s1, gamma, dtype):
    """train_gcn_dqn.py:113-124 on S complete graphs of N nodes with the three-layer network."""
    S, N, _ = s.shape
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in O.gat3_unflatten(p).items()}
    T = {k: v.to(dtype) for k, v in O.gat3_unflatten(tgt).items()}
    mult = O.multiplicity_complete(S, N).to(dtype)
    x = O.node_features(s[..., :2], s[..., 2:4]).to(dtype)
    xn = O.node_features(s1[..., :2], s1[..., 2:4]).to(dtype)
    values = O.gat3_q_forward_dense(P, x, mult).reshape(S * N, -1).gather(1, actions.reshape(-1, 1).long())
    with torch.no_grad():
        next_values = O.gat3_q_forward_dense(T, xn, mult).reshape(S * N, -1).max(dim=1)[0]
    target = rewards.reshape(-1).to(dtype) + gamma * next_values
    torch.nn.MSELoss()(values, target.unsqueeze(1)).backward()
    return _flat_grad(P)


def test_autograd_runs_the_reference_training_step(sw, golden_weights):
    """train_gcn_dqn.py:113-126 as written, with GAT3(autograd=True) as the model."""
    N, S, gamma = 8, 32, 0.99
    p, tgt = _weights(golden_weights, 4), _weights(golden_weights, 8)
    model, plain, target_model = _model(sw, p, autograd=True), _model(sw, p), _model(sw, tgt)
    g = torch.Generator().manual_seed(7)
    s = torch.randn(S, N, 4, generator=g) * 0.4
    s1 = torch.randn(S, N, 4, generator=g) * 0.4
    actions = torch.randint(0, 9, (S * N,), generator=g)
    rewards = torch.randn(S * N, generator=g)
    obs = sw.Batch.from_data_list([sw.create_graph_from_observations(_obs(s[i:i + 1])) for i in range(S)])
    nextObs = sw.Batch.from_data_list([sw.create_graph_from_observations(_obs(s1[i:i + 1])) for i in range(S)])
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = {k: q.detach().clone() for k, q in model.named_parameters()}

    q_on = model(obs)
    assert q_on.requires_grad
    assert torch.equal(q_on.detach(), plain(obs)), "Q with autograd on and off"

    optimizer.zero_grad()
    values = model(obs).gather(1, actions.cuda().unsqueeze(1))
    with torch.no_grad():
        nextValues = target_model(nextObs).max(dim=1)[0].detach()
    targetValues = rewards.cuda() + (gamma * nextValues)
    loss = torch.nn.MSELoss()(values, targetValues.unsqueeze(1))
    loss.backward()
    named = dict(model.named_parameters())
    for k, shape in O.GAT3_PARAM_ORDER:
        assert named[k].grad is not None and tuple(named[k].grad.shape) == tuple(named[k].shape) == tuple(shape), k
        assert named[k].grad.device == named[k].device, k
    got = _named_grad(model)
    g64 = _oracle_td_grad(p, tgt, s, actions, rewards, s1, gamma, torch.float64)
    g32 = _oracle_td_grad(p, tgt, s, actions, rewards, s1, gamma, torch.float32)
    err = _metric(got, g64)
    rec = record("gat3 autograd TD grad", dict(n=NP3, max_abs=float((got.double() - g64).abs().max()), max_rel=err),
                 oracle_fp32=_metric(g32, g64), tol_rel=GRAD_TOL)
    print(rec)
    assert err < GRAD_TOL, err
    nonzero = {k: bool(q.grad.any()) for k, q in model.named_parameters()}
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
    optimizer.step()
    assert any(nonzero.values())
    for k, q in model.named_parameters():   # every parameter with a non-zero gradient moves, and no other
        assert torch.equal(before[k], q.detach()) != nonzero[k], k
    # the forward sees the new weights
    assert not torch.equal(model(obs).detach(), q_on.detach())


# ------------------------------------------------------------------ 5. an edge_index batch
def test_autograd_on_an_edge_index_batch(sw, golden_weights):
    """A batch with an explicit PyG edge_index (the dense path through edges_to_mult)."""
    N, G, k = 6, 5, 3
    p = _weights(golden_weights, 4)
    model = _model(sw, p, autograd=True)
    gen = torch.Generator().manual_seed(100 * N + G)
    s = torch.randn(G, N, 4, generator=gen) * 0.4
    dq = torch.randn(G * N, 9, generator=gen)
    x = O.node_features(s[..., :2], s[..., 2:4])
    batch = sw.Batch.from_data_list([sw.Data(x[i], O.knn_edge_index(s[i, :, :2], k)) for i in range(G)])
    assert batch.swarm is None
    q = model(batch)
    (q * dq.cuda()).sum().backward()
    got = _named_grad(model)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        P = {kk: v.to(dtype).clone().requires_grad_(True) for kk, v in O.gat3_unflatten(p).items()}
        qr = O.gat3_q_forward_edges(P, x.reshape(G * N, 7).to(dtype), batch.edge_index)
        (qr * dq.to(dtype)).sum().backward()
        grads[dtype] = _flat_grad(P)
    g64 = grads[torch.float64]
    err = _metric(got, g64)
    rec = record("gat3 autograd edge_index grad", dict(n=NP3, max_abs=float((got.double() - g64).abs().max()), max_rel=err),
                 oracle_fp32=_metric(grads[torch.float32], g64), tol_rel=GRAD_TOL)
    print(rec)
    assert err < GRAD_TOL, err


# ------------------------------------------------------------------ 6. the remaining semantics
def test_autograd_is_opt_in(sw, golden_weights):
    p = _weights(golden_weights, 4)
    s = torch.randn(3, 5, 4, generator=torch.Generator().manual_seed(1)) * 0.4
    batch = sw.create_graph_from_observations(_obs(s))
    assert not _model(sw, p)(batch).requires_grad
    model = _model(sw, p, autograd=True)
    with torch.no_grad():
        assert not model(batch).requires_grad
    assert model(batch).requires_grad
    for q in model.parameters():
        q.requires_grad_(False)
    assert not model(batch).requires_grad
    # some parameters frozen: they get no gradient, the others do
    model = _model(sw, p, autograd=True)
    model.conv2.lin.weight.requires_grad_(False)
    model.lin1.bias.requires_grad_(False)
    model(batch).sum().backward()
    for k, q in model.named_parameters():
        assert (q.grad is None) == (k in ("conv2.lin.weight", "lin1.bias")), k


def test_autograd_empty_batch_gives_zero_gradients(sw, golden_weights):
    model = _model(sw, _weights(golden_weights, 4), autograd=True)
    batch = sw.create_graph_from_observations(torch.zeros(0, 5, 6))
    q = model(batch)
    assert tuple(q.shape) == (0, 9) and q.requires_grad
    q.sum().backward()
    for k, q_ in model.named_parameters():
        assert q_.grad is not None and q_.grad.shape == q_.shape and not q_.grad.any(), k


def test_from_state_dict_returns_a_trainable_gat3(sw, golden_weights):
    sd = O.gat3_unflatten(_weights(golden_weights, 4))
    m = sw.GCN.from_state_dict(sd, autograd=True)
    assert isinstance(m, sw.GAT3) and m.autograd is True and m.layers == 3 and m.net == "gat3"
    s = torch.randn(2, 5, 4, generator=torch.Generator().manual_seed(2)) * 0.4
    q = m(sw.create_graph_from_observations(_obs(s)))
    assert q.requires_grad and torch.equal(q.detach(), sw.GCN.from_state_dict(sd)(sw.create_graph_from_observations(_obs(s))))
