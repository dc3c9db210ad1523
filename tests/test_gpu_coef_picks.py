"""The in-edge coefficients as each lane's own picks (swarm_dl.h CoefPick, sel4).

dl_forward forms, per target node, only the coefficients its lane reads: the column picks (the
aggregate's B operand and the backward's cm image) and the row picks (bwd_attention's edges), each a
select among four candidates plus one same-graph mask; on the complete graph the multiplicity is
carried as a predicate.  A wrong candidate, a wrong mask or a neighbour graph leaking into a wave
that holds two graphs changes which source a coefficient weighs.  With 1,673 distinct weights and
random positions every coefficient is distinct, so any such error moves Q and the gradient far
outside the oracle bounds used here (tests/test_gpu_parity.py's Q bound, tests/test_gpu_parity_large.py's
gradient bounds, both imported, neither altered).

Shapes: 5 envs, a TD batch of S = 3 graphs, a replay ring of 2 slots.  The odd counts leave one graph
slot of the last TD wave as padding beside a live graph, and one TD block holds graphs of the slot
being written (pre path / hand-off) beside ordinary ones.  N = 5, 8: two 8-slot graphs per TD wave
and the 8-slot acting kernels; N = 9, 16: one 16-slot graph per wave; N = 17: two column tiles
(32 slots), through the 3-launch tick's TD kernel.  GAT and GCN; complete, kNN-3 and radius graphs.

The oracle's autograd has the GCN variant on complete graphs only, so the gradient of GCN on kNN and
radius graphs has no independent reference here.  What the picks feed into it is the cm image, a copy
of the forward's column picks, and those are held to the oracle by the Q-forward cases of GCN on kNN
and radius graphs; the fused-against-3-launch cases of these variants compare one code path with itself.
"""
import functools

import pytest
import torch

from oracle import swarm_oracle as O
from tests.test_gpu_parity import Q_ULP, _fill_replay, _rand_state
from tests.test_gpu_prologue_image import _distinct_weights

B, S, SLOTS = 5, 3, 2
K, R_Q, R_TD = 3, 0.3, 0.5          # kNN-3; the radii of test_q_forward_parity / test_td_update_parity
AGENTS = (5, 8, 9, 16, 17)
VARIANTS = [("complete", "gat"), ("complete", "gcn"), ("knn", "gat"), ("knn", "gcn"), ("radius", "gat"), ("radius", "gcn")]
Q_CASES = [(N, g, c) for N in AGENTS for g, c in VARIANTS]
# the oracle's autograd has the GCN variant on complete graphs only
TD_CASES = [(N, g, c) for N, g, c in Q_CASES if c == "gat" or g == "complete"]
TICK_CASES = [(N, g, c) for N, g, c in Q_CASES if N <= 16]   # the fused tick's agent counts
# batch indices into the ring of SLOTS * B graphs: slot 0 (the slot being written: pre path), slot 1, slot 0
IDX = (1, 7, 3)


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _weights():
    p = _distinct_weights()
    return p, p.flip(0).contiguous()   # online, target


def _mult(pos, graph, radius):
    if graph == "complete":
        return O.multiplicity_complete(pos.shape[0], pos.shape[1])
    if graph == "knn":
        return O.multiplicity_knn(O.knn_sets(pos, K))
    return O.multiplicity_radius(O.radius_sets(pos, radius))


@functools.lru_cache(maxsize=None)
def _q_reference(N, graph, conv, dtype=torch.float32):
    """(pos, vel, oracle Q [B, N, 9]) of the Q-forward case; computed once per case"""
    pos, vel = _rand_state(B, N, 70 + N)
    P = {k: v.to(dtype) for k, v in O.unflatten_params(_weights()[0]).items()}
    x, mult = O.node_features(pos, vel).to(dtype), _mult(pos, graph, R_Q).to(dtype)
    q = (O.q_forward_dense if conv == "gat" else O.gcn_conv_dense)(P, x, mult)
    return pos, vel, q


def _replay_rows(N):
    """the ring's content (tests/test_gpu_parity.py _fill_replay, seed 30 + N), on the CPU"""
    g = torch.Generator().manual_seed(30 + N)
    s = torch.randn(SLOTS, B, N, 4, generator=g) * 0.4
    s1 = torch.randn(SLOTS, B, N, 4, generator=g) * 0.4
    r = torch.randn(SLOTS, B, N, generator=g)
    a = torch.randint(0, 9, (SLOTS, B, N), generator=g)
    return s, s1, r, a


@functools.lru_cache(maxsize=None)
def _td_reference(N, graph, conv):
    """the fp32 oracle's gradient five ways and the float64 one (test_gpu_parity_large.py
    oracle_grad_orders) on the graphs IDX; computed once per case"""
    from tests.test_gpu_parity_large import oracle_grad_orders
    p, tgt = _weights()
    s, s1, r, a = _replay_rows(N)
    idx = torch.tensor(IDX)
    slot, env = idx // B, idx % B
    edge_fn = None
    if graph == "knn":
        edge_fn = lambda ss: torch.cat([O.knn_edge_index(ss[g, :, :2], K) + g * N for g in range(ss.shape[0])], dim=1)  # noqa: E731
    elif graph == "radius":
        edge_fn = lambda ss: torch.cat([O.radius_edge_index(ss[g, :, :2], R_TD) + g * N for g in range(ss.shape[0])], dim=1)  # noqa: E731
    _, g32s, _, g64 = oracle_grad_orders(p, tgt, s[slot, env], a[slot, env], r[slot, env], s1[slot, env], conv=conv,
                                         seed=S + N, edge_fn=edge_fn)
    return g32s, g64


# ---------------------------------------------------------------- CPU: the oracle alone, on these inputs
@pytest.mark.parametrize("N,graph,conv", Q_CASES)
def test_oracle_q_is_inside_the_q_bound(N, graph, conv):
    """the fp32 oracle against its own float64 evaluation, under the bound the GPU is held to"""
    from tests.conftest import assert_close_ulp
    q32, q64 = _q_reference(N, graph, conv)[2], _q_reference(N, graph, conv, torch.float64)[2]
    assert_close_ulp(q32, q64, Q_ULP, f"coef picks oracle Q N={N} {graph} {conv}", scale=1.0, rel_floor=1e-5)


@pytest.mark.parametrize("N,graph,conv", TD_CASES)
def test_oracle_gradient_is_inside_the_gradient_bounds(N, graph, conv):
    from tests.test_gpu_parity_large import _grad_bound_check
    g32s, g64 = _td_reference(N, graph, conv)
    assert float(g64.abs().max()) > 0.0
    for i, g in enumerate(g32s):
        _grad_bound_check(f"coef picks oracle evaluation {i} N={N} {graph} {conv}", g, g32s, g64)


# ---------------------------------------------------------------- GPU
def _engine(sw, N, graph, conv, radius, params=None, seed=13):
    return sw.SwarmEngine("GoTo", N, B, seed=seed, params=_weights()[0] if params is None else params, batch=S, eps=0.3,
                          update_target_every=1000, replay_capacity=SLOTS * B, graph=graph, knn_k=K, conv=conv,
                          radius=radius)


@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", Q_CASES)
def test_q_forward_against_the_oracle(sw, N, graph, conv):
    from swarm_amd._lib import call, ptr
    from tests.conftest import assert_close_ulp
    pos, vel, ref = _q_reference(N, graph, conv)
    eng = _engine(sw, N, graph, conv, R_Q)
    x = O.node_features(pos, vel).reshape(B * N, 7).contiguous().cuda()
    q = torch.zeros(B * N, 9, device="cuda")
    call(eng.lib, "swarm_q_forward", eng.cfg, ptr(eng.params), ptr(x), None, ptr(q))
    torch.cuda.synchronize()
    assert_close_ulp(q.cpu().view(B, N, 9), ref, Q_ULP, f"coef picks Q N={N} {graph} {conv}", scale=1.0, rel_floor=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", TD_CASES)
def test_td_gradient_against_the_oracle_autograd(sw, N, graph, conv):
    """swarm_td_grad + swarm_grad_reduce on three graphs of the ring (two of the slot being written:
    their waves take the pre path) against the oracle's autograd"""
    from tests.test_gpu_parity_large import _grad_bound_check
    g32s, g64 = _td_reference(N, graph, conv)
    eng = _engine(sw, N, graph, conv, R_TD)
    eng.target.copy_(_weights()[1].cuda())
    _fill_replay(eng, 30 + N)
    s, s1, r, a = _replay_rows(N)
    assert torch.equal(eng.rep_s.cpu(), s) and torch.equal(eng.rep_a.cpu().long(), a), "the reference's rows"
    eng.td_grad(sample_in=torch.tensor(IDX, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    _grad_bound_check(f"coef picks TD N={N} {graph} {conv}", eng.grad.cpu()[:O.N_PARAMS], g32s, g64)


@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", TICK_CASES)
def test_fused_tick_equals_three_launch_tick(sw, N, graph, conv):
    """Q, gradient and weights of swarm_train_tick bitwise equal to the 3-launch tick's, every tick;
    with a ring of two slots about half of each batch comes through the hand-off records"""
    a, b = _engine(sw, N, graph, conv, R_TD), _engine(sw, N, graph, conv, R_TD)
    assert a.fused
    for e in (a, b):
        e.set_state(*_rand_state(B, N, 50 + N))
    n_cur = 0
    for t in range(4):
        a.train_tick(full_out=True)
        b.train_tick3(full_out=True)
        torch.cuda.synchronize()
        ca = a.read_ctrl()
        assert ca == b.read_ctrl(), t
        assert torch.equal(a.q, b.q) and torch.equal(a.actions, b.actions), t
        assert torch.equal(a.grad, b.grad), t
        if ca["trained"]:
            assert torch.equal(a.samples, b.samples), t
            assert float(a.grad[:O.N_PARAMS].abs().max()) > 0.0
            n_cur += int(((a.samples // B) == (ca["write_slot"] - 1) % SLOTS).sum())
    a.flush()
    b.flush()
    torch.cuda.synchronize()
    assert a.handoff_errors() == 0
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert not torch.equal(a.params.cpu(), _weights()[0]), "steps were applied"
    assert n_cur > 0, "some graphs came from the tick's own slot"
