"""GPU parity of swarm_q_backward (the backward of GCN.forward for a caller's dL/dQ) and of the
``GCN(autograd=True)`` binding, against the oracle's torch autograd evaluated in float64 from the
same fp32 inputs.

Bar: the project's gradient bar (tests/test_gpu_parity.py test_td_update_parity):
max|g_gpu - g64| / max(max|g64|, 1e-3) < 2e-5.  On the CPU the oracle's own fp32 evaluation
stays at or below 2.8e-6 in that metric on every case below."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import swarm_oracle as O
from tests.conftest import record

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-5
SCEN = {"go_to": O.SCENARIO_GOTO, "obstacle_avoidance": O.SCENARIO_OA}
GRAPH = {"complete": 0, "knn": 1, "dense": 2, "radius": 3}
RADIUS = 0.5

# (scenario, N, B, graph, k, conv, holes): holes = a node with no in-edge and a graph with no edge
CASES = [
    ("go_to", 1, 3, "complete", 0, "gat", False), ("go_to", 2, 9, "complete", 0, "gat", False),   # smallest graphs
    ("go_to", 5, 7, "complete", 0, "gat", False),        # last block partly filled, 8-slot graphs
    ("go_to", 8, 32, "complete", 0, "gat", False), ("go_to", 8, 33, "complete", 0, "gcn", False),   # a row of slabs + 1
    ("go_to", 8, 260, "complete", 0, "gat", False),      # 65 slabs: the reduce's groups take two slabs each
    ("go_to", 9, 5, "complete", 0, "gcn", False), ("go_to", 16, 4, "complete", 0, "gat", False),   # 16-slot graphs
    ("obstacle_avoidance", 17, 3, "dense", 0, "gcn", False), ("obstacle_avoidance", 29, 2, "complete", 0, "gat", False),
    ("obstacle_avoidance", 32, 2, "knn", 10, "gat", False),   # 32-slot graphs
    ("obstacle_avoidance", 12, 5, "knn", 5, "gat", False), ("go_to", 20, 3, "knn", 10, "gat", False),
    ("go_to", 8, 6, "radius", 0, "gat", False),          # built graphs
    ("go_to", 6, 4, "dense", 0, "gat", False),           # multiplicities up to 3
    ("go_to", 6, 3, "dense", 0, "gat", True), ("obstacle_avoidance", 6, 3, "dense", 0, "gcn", True),
]


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _weights(golden_weights, scen, seed=5):
    return torch.tensor(golden_weights[scen][seed])


def _inputs(N, B, graph, holes=False):
    """The issue's inputs: state, features, (dense) multiplicities, dL/dQ from one generator."""
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


def _oracle_grad(p, x, mult, dq, conv, dtype=torch.float64):
    """d (q * dq).sum() / d params by the oracle's autograd on the dense multiplicity form."""
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in O.unflatten_params(p).items()}
    fwd = O.q_forward_dense if conv == "gat" else O.gcn_conv_dense
    q = fwd(P, x.to(dtype), mult.to(dtype))
    (q * dq.to(dtype)).sum().backward()
    return torch.cat([(P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).reshape(-1)
                      for k, _ in O.PARAM_ORDER])


@functools.lru_cache(maxsize=None)
def _case_inputs(N, B, graph, k, holes):
    s, x, mult, dq = _inputs(N, B, graph, holes)
    if graph != "dense":   # the multiplicities the kernel builds itself, for the oracle
        og = {"complete": O.GRAPH_COMPLETE, "knn": O.GRAPH_KNN, "radius": O.GRAPH_RADIUS}[graph]
        mult = O.graph_multiplicity(s[..., :2], og, k, RADIUS)
    return s, x, mult, dq


def _metric(g, g64):
    return ((g.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-3)).item()


def _q_backward(scen, N, B, graph, k, conv, p, x, mult, dq):
    """swarm_q_backward through the C ABI, workspace and grad pre-filled with NaN."""
    import swarm_amd._lib as L
    lib = L.load()
    cfg = L.SwarmConfig(B, N, SCEN[scen], GRAPH[graph], k, L.CONV_GAT if conv == "gat" else L.CONV_GCN, 0, 0, 0,
                        RADIUS if graph == "radius" else 0.0, L.NET_GCN)
    n_ws = lib.swarm_td_workspace_floats(ctypes.byref(cfg), B)
    assert n_ws > 0
    dev = dict(device="cuda", dtype=torch.float32)
    ws = torch.full((n_ws,), float("nan"), **dev)
    grad = torch.full((L.GRAD_FLOATS,), float("nan"), **dev)
    pd = p.to(**dev).contiguous()
    xd = x.reshape(B * N, 7).to(**dev).contiguous()
    dqd = dq.reshape(B * N, 9).to(**dev).contiguous()
    md = mult.to(torch.uint8).cuda().contiguous() if graph == "dense" else None
    rc = lib.swarm_q_backward(ctypes.byref(cfg), L.ptr(pd), L.ptr(xd), L.ptr(md), L.ptr(dqd), L.ptr(ws), L.ptr(grad),
                              L.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return grad.cpu()


def _norm_partials(g):
    """The clip norm's 105 group partials of a gradient, in the header's fixed order (fp32)."""
    sq = np.zeros(105 * 16, dtype=np.float32)
    gg = g.numpy().astype(np.float32)
    sq[:O.N_PARAMS] = gg * gg
    sq = sq.reshape(-1, 4)
    d = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
    d = d.reshape(105, 4)
    return (d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3])


@pytest.mark.parametrize("scen,N,B,graph,k,conv,holes", CASES)
def test_q_backward_parity(sw, golden_weights, scen, N, B, graph, k, conv, holes):
    import swarm_amd._lib as L
    p = _weights(golden_weights, scen)
    s, x, mult, dq = _case_inputs(N, B, graph, k, holes)
    g64 = _oracle_grad(p, x, mult, dq, conv)
    g32 = _oracle_grad(p, x, mult, dq, conv, torch.float32)
    out = _q_backward(scen, N, B, graph, k, conv, p, x, mult, dq)
    g = out[:O.N_PARAMS]
    assert torch.isfinite(out[:O.N_PARAMS + 1]).all(), "an unwritten slab column (NaN workspace) or a non-finite sum"
    err = _metric(g, g64)
    rec = record(f"q_backward grad {scen} N={N} B={B} {graph} {conv}" + (" holes" if holes else ""),
                 dict(n=O.N_PARAMS, max_abs=float((g.double() - g64).abs().max()), max_rel=err),
                 oracle_fp32=_metric(g32, g64), tol_rel=GRAD_TOL)
    assert err < GRAD_TOL, f"gradient: {err:.3e} (oracle fp32 {rec['oracle_fp32']:.3e})"
    assert out[O.N_PARAMS].item() == 0.0
    got = out[L.GRAD_SQ_BASE:L.GRAD_SQ_BASE + 105].numpy()
    assert np.array_equal(got.view(np.uint32), _norm_partials(g).view(np.uint32)), "norm partials"
    if conv == "gcn":
        assert (g[:64] == 0).all(), "attention columns under GCNConv"


def test_q_backward_is_deterministic(sw, golden_weights):
    p = _weights(golden_weights, "go_to")
    s, x, mult, dq = _case_inputs(8, 33, "complete", 0, False)
    a = _q_backward("go_to", 8, 33, "complete", 0, "gat", p, x, mult, dq)
    b = _q_backward("go_to", 8, 33, "complete", 0, "gat", p, x, mult, dq)
    assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


def test_q_backward_agrees_with_td_kernel(sw, golden_weights):
    """The shipped TD kernel's gradient (test_td_update_parity's first case) equals swarm_q_backward
    fed the same loss's dL/dQ: each is within 2e-5 of the oracle, so 4e-5 of each other."""
    from tests.test_gpu_parity import _fill_replay
    scen, N, S, B = "go_to", 8, 32, 16
    cap = max(4, -(-S // B))
    p, tgt = _weights(golden_weights, scen, 5), _weights(golden_weights, scen, 6)
    eng = sw.SwarmEngine(scen, N, B, seed=2, params=p, batch=S, replay_capacity=cap * B, update_target_every=1000,
                         graph="complete", knn_k=1, conv="gat", radius=0.5)
    eng.target.copy_(tgt.cuda())
    _fill_replay(eng, S)
    idx = torch.randperm(cap * B, generator=torch.Generator().manual_seed(S))[:S].to(torch.int32)
    eng.td_grad(sample_in=idx.cuda())
    torch.cuda.synchronize()
    g_td = eng.grad.cpu()[:O.N_PARAMS]
    slot, env = (idx // B).long(), (idx % B).long()
    s = eng.rep_s.cpu()[slot, env]
    s1 = eng.rep_s1.cpu()[slot, env]
    a = eng.rep_a.cpu()[slot, env].long()
    r = eng.rep_r.cpu()[slot, env]
    ref = O.td_step(p, tgt, torch.zeros_like(p), torch.zeros_like(p), 0, s, a, r, s1)
    dq = torch.zeros(S * N, 9)
    dq[torch.arange(S * N), a.reshape(-1)] = (2.0 / (S * N)) * (ref["values"] - ref["target"]).float()
    x = O.node_features(s[..., :2], s[..., 2:4])
    g_q = _q_backward(scen, N, S, "complete", 0, "gat", p, x, None, dq)[:O.N_PARAMS]
    err = ((g_q - g_td).abs().max() / g_td.abs().max().clamp_min(1e-3)).item()
    record("q_backward vs td_grad", dict(n=O.N_PARAMS, max_abs=float((g_q - g_td).abs().max()), max_rel=err),
           tol_rel=2 * GRAD_TOL)
    assert err < 2 * GRAD_TOL, err


def _obs(s):
    """[B, N, 6] observations (pos, vel, goal) of states [B, N, 4]."""
    return O.node_features(s[..., :2], s[..., 2:4])[..., :6]


def _load(model, flat):
    model.load_state_dict(O.unflatten_params(flat))
    return model


def test_autograd_runs_the_reference_training_step(sw, golden_weights):
    """train_gcn_dqn.py:113-126 as written, with the drop-in classes."""
    N, S, gamma = 8, 32, 0.99
    p, tgt = _weights(golden_weights, "go_to", 5), _weights(golden_weights, "go_to", 6)
    model = _load(sw.GCN(7, 32, 9, autograd=True), p)
    plain = _load(sw.GCN(7, 32, 9), p)
    target_model = _load(sw.GCN(7, 32, 9), tgt)
    g = torch.Generator().manual_seed(7)
    s = torch.randn(S, N, 4, generator=g) * 0.4
    s1 = torch.randn(S, N, 4, generator=g) * 0.4
    actions = torch.randint(0, 9, (S * N,), generator=g)
    rewards = torch.randn(S * N, generator=g)
    obs = sw.Batch.from_data_list([sw.create_graph_from_observations(_obs(s[i:i + 1])) for i in range(S)])
    nextObs = sw.Batch.from_data_list([sw.create_graph_from_observations(_obs(s1[i:i + 1])) for i in range(S)])
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = [q.detach().clone() for q in model.parameters()]

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
    for k, shape in O.PARAM_ORDER:
        assert named[k].grad is not None and tuple(named[k].grad.shape) == tuple(named[k].shape) == tuple(shape), k
        assert named[k].grad.device == named[k].device, k
    got = torch.cat([named[k].grad.reshape(-1).cpu() for k, _ in O.PARAM_ORDER])
    _, g64, _, _ = O.td_loss_grad(p, tgt, s, actions.reshape(S, N), rewards.reshape(S, N), s1, gamma,
                                  dtype=torch.float64)
    err = _metric(got, g64)
    record("autograd TD grad", dict(n=O.N_PARAMS, max_abs=float((got.double() - g64).abs().max()), max_rel=err),
           tol_rel=GRAD_TOL)
    assert err < GRAD_TOL, err
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
    optimizer.step()
    assert all(not torch.equal(b, q.detach()) for b, q in zip(before, model.parameters()))
    # the forward sees the new weights
    assert not torch.equal(model(obs).detach(), q_on.detach())


def test_autograd_on_an_edge_index_batch(sw, golden_weights):
    """A batch with an explicit PyG edge_index (the dense path through edges_to_mult)."""
    N, G, k = 6, 5, 3
    p = _weights(golden_weights, "go_to", 5)
    model = _load(sw.GCN(7, 32, 9, autograd=True), p)
    gen = torch.Generator().manual_seed(100 * N + G)
    s = torch.randn(G, N, 4, generator=gen) * 0.4
    dq = torch.randn(G * N, 9, generator=gen)
    x = O.node_features(s[..., :2], s[..., 2:4])
    datas = [sw.Data(x[i], O.knn_edge_index(s[i, :, :2], k)) for i in range(G)]
    batch = sw.Batch.from_data_list(datas)
    assert batch.swarm is None
    q = model(batch)
    (q * dq.cuda()).sum().backward()
    named = dict(model.named_parameters())
    got = torch.cat([named[kk].grad.reshape(-1).cpu() for kk, _ in O.PARAM_ORDER])
    grads = {}
    for dtype in (torch.float64, torch.float32):
        P = {kk: v.to(dtype).clone().requires_grad_(True) for kk, v in O.unflatten_params(p).items()}
        qr = O.q_forward_edges(P, x.reshape(G * N, 7).to(dtype), batch.edge_index)
        (qr * dq.to(dtype)).sum().backward()
        grads[dtype] = torch.cat([P[kk].grad.reshape(-1) for kk, _ in O.PARAM_ORDER])
    g64 = grads[torch.float64]
    err = _metric(got, g64)
    record("autograd edge_index grad", dict(n=O.N_PARAMS, max_abs=float((got.double() - g64).abs().max()), max_rel=err),
           oracle_fp32=_metric(grads[torch.float32], g64), tol_rel=GRAD_TOL)
    assert err < GRAD_TOL, err


def test_autograd_is_opt_in(sw, golden_weights):
    p = _weights(golden_weights, "go_to", 5)
    s = torch.randn(3, 5, 4, generator=torch.Generator().manual_seed(1)) * 0.4
    batch = sw.create_graph_from_observations(_obs(s))
    assert not _load(sw.GCN(7, 32, 9), p)(batch).requires_grad
    model = _load(sw.GCN(7, 32, 9, autograd=True), p)
    with torch.no_grad():
        assert not model(batch).requires_grad
    assert model(batch).requires_grad
    for q in model.parameters():
        q.requires_grad_(False)
    assert not model(batch).requires_grad


def test_autograd_empty_batch_gives_zero_gradients(sw, golden_weights):
    model = _load(sw.GCN(7, 32, 9, autograd=True), _weights(golden_weights, "go_to", 5))
    batch = sw.create_graph_from_observations(torch.zeros(0, 5, 6))
    q = model(batch)
    assert tuple(q.shape) == (0, 9) and q.requires_grad
    q.sum().backward()
    for k, q_ in model.named_parameters():
        assert q_.grad is not None and q_.grad.shape == q_.shape and not q_.grad.any(), k
