"""The forward's weight-image operands as one early batch of registers (swarm_dl.h DFrag).

The fused tick's kernels read every operand of dl_forward that depends only on the weight image
and the lane (the lin0 / lin1 / lin2 A fragments, the attention vectors, the three biases) in one
batch right behind the image's barrier, mask them in registers, and write a node's Q as one 16-B
store per lane.  A misplaced fragment (a wrong row, k tile or row group), a wrong mask (feature 7,
action rows 9..15, b2 words 9..11) or a clobbered Q word moves Q, and through it the actions, the
TD target and the gradient.  With 1,673 pairwise distinct weights (tests/test_gpu_prologue_image.py
_distinct_weights, as tests/test_gpu_coef_picks.py builds them) all nine b2 words and every fragment
row differ, so any such error lies far outside the oracle bounds used here: tests/test_gpu_parity.py's
Q bound and tests/test_gpu_parity_large.py's gradient bounds, both imported, neither altered.

Which kernel runs which form: the fused tick (swarm_train_tick) takes the fragments in its acting,
online and target waves; swarm_q_forward, swarm_td_grad and the 3-launch tick read each operand in
front of its use, as before.  So the chain is: the unfragmented kernels against the oracle (Q
forward, TD gradient), the fused tick's Q of its first tick against the oracle directly, and the
fused tick bitwise against the 3-launch tick over six ticks (Q, actions, rewards, gradient, control
block, weights, moments, ring).

Shapes (tests/test_gpu_coef_picks.py's, whose cached references are shared): 5 envs, S = 3, a ring
of two slots, so most draws wait on a hand-off; N = 5, 8 (8-slot acting waves, two graphs per TD
wave, idle lanes inside a graph at N = 5) and N = 9, 16 (16-slot acting waves, idle lanes past a
graph at N = 9); GAT and GCN on the complete graph, and radius + GAT at N <= 8, the tick's other
instance.  The full [B, N, 9] Q is compared: action 8 (the lone word of row group p == 2) and agents
N - 1 and 0 of neighbouring envs are part of it, and are checked to be pairwise distinct in the
reference so that a shifted word cannot pass.
"""
import pytest
import torch

from oracle import swarm_oracle as O
from tests.test_gpu_coef_picks import (B, IDX, R_Q, R_TD, S, SLOTS, _engine, _q_reference, _replay_rows, _td_reference,
                                       _weights)
from tests.test_gpu_parity import Q_ULP, _fill_replay, _rand_state

AGENTS = (5, 8, 9, 16)
CASES = ([(N, "complete", c) for N in AGENTS for c in ("gat", "gcn")] +
         [(N, "radius", "gat") for N in AGENTS if N <= 8])
SYNC_EVERY, TICKS = 2, 6


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _check_q(q, ref, what):
    from tests.conftest import assert_close_ulp
    N = ref.shape[1]
    # what a shifted or clobbered word would have to equal: its neighbours in the row, and the
    # rows on either side of an env boundary
    assert (ref[..., 8] != ref[..., 7]).all() and (ref[:-1, N - 1] != ref[1:, 0]).all(), "distinct reference words"
    assert_close_ulp(q, ref, Q_ULP, what, scale=1.0, rel_floor=1e-5)


# ---------------------------------------------------------------- CPU: the oracle alone, on these inputs
@pytest.mark.parametrize("N,graph,conv", CASES)
def test_oracle_q_is_inside_the_q_bound(N, graph, conv):
    """the fp32 oracle against its own float64 evaluation, under the bound the GPU is held to"""
    _check_q(_q_reference(N, graph, conv)[2], _q_reference(N, graph, conv, torch.float64)[2],
             f"fragments oracle Q N={N} {graph} {conv}")


@pytest.mark.parametrize("N,graph,conv", CASES)
def test_oracle_gradient_is_inside_the_gradient_bounds(N, graph, conv):
    from tests.test_gpu_parity_large import _grad_bound_check
    g32s, g64 = _td_reference(N, graph, conv)
    assert float(g64.abs().max()) > 0.0
    for i, g in enumerate(g32s):
        _grad_bound_check(f"fragments oracle evaluation {i} N={N} {graph} {conv}", g, g32s, g64)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", CASES)
def test_q_forward_against_the_oracle(sw, N, graph, conv):
    from swarm_amd._lib import call, ptr
    pos, vel, ref = _q_reference(N, graph, conv)
    eng = _engine(sw, N, graph, conv, R_Q)
    x = O.node_features(pos, vel).reshape(B * N, 7).contiguous().cuda()
    q = torch.zeros(B * N, 9, device="cuda")
    call(eng.lib, "swarm_q_forward", eng.cfg, ptr(eng.params), ptr(x), None, ptr(q))
    torch.cuda.synchronize()
    _check_q(q.cpu().view(B, N, 9), ref, f"fragments Q N={N} {graph} {conv}")


@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", CASES)
def test_fused_tick_q_against_the_oracle(sw, N, graph, conv):
    """the acting waves' forward with fragments and the one-store Q epilogue: the first fused
    tick's Q (no optimizer step is pending yet, so the weights are the ones given)"""
    pos, vel, ref = _q_reference(N, graph, conv)
    eng = _engine(sw, N, graph, conv, R_Q)
    assert eng.fused
    eng.set_state(pos, vel)
    eng.train_tick(full_out=True)
    torch.cuda.synchronize()
    assert eng.handoff_errors() == 0
    _check_q(eng.q.cpu(), ref, f"fragments fused tick Q N={N} {graph} {conv}")


@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", CASES)
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
    _grad_bound_check(f"fragments TD N={N} {graph} {conv}", eng.grad.cpu()[:O.N_PARAMS], g32s, g64)


@pytest.mark.gpu
@pytest.mark.parametrize("N,graph,conv", CASES)
def test_fused_tick_equals_three_launch_tick(sw, N, graph, conv):
    """six ticks with a target sync every second one: the fused tick (fragments in its acting, online
    and target waves; on a sync tick the target image is written before the batch is read) bitwise
    equal to the 3-launch tick (no fragments) in everything a tick leaves behind"""
    kw = dict(n_agents=N, n_envs=B, seed=13, params=_weights()[0], batch=S, eps=0.3, update_target_every=SYNC_EVERY,
              replay_capacity=SLOTS * B, graph=graph, knn_k=3, conv=conv, radius=R_TD)
    a, b = sw.SwarmEngine("GoTo", **kw), sw.SwarmEngine("GoTo", **kw)
    assert a.fused
    for e in (a, b):
        e.target.copy_(_weights()[1].cuda())   # distinct from the online weights until the first sync
        e.set_state(*_rand_state(B, N, 50 + N))
    n_cur = 0
    for t in range(TICKS):
        a.train_tick(full_out=True)
        b.train_tick3(full_out=True)
        torch.cuda.synchronize()
        ca = a.read_ctrl()
        assert ca == b.read_ctrl(), t
        assert torch.equal(a.q, b.q) and torch.equal(a.actions, b.actions) and torch.equal(a.reward, b.reward), t
        assert torch.equal(a.state, b.state), t
        assert torch.equal(a.grad, b.grad), t
        if ca["trained"]:
            assert torch.equal(a.samples, b.samples), t
            assert float(a.grad[:O.N_PARAMS].abs().max()) > 0.0
            n_cur += int(((a.samples // B) == (ca["write_slot"] - 1) % SLOTS).sum())
    assert torch.equal(a.target, b.target), "the synced target"
    assert not torch.equal(a.target.cpu(), _weights()[1]), "a target sync happened"
    a.flush()
    b.flush()
    torch.cuda.synchronize()
    assert a.handoff_errors() == 0
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert torch.equal(a.rep_s, b.rep_s) and torch.equal(a.rep_s1, b.rep_s1), "ring: s, s'"
    assert torch.equal(a.rep_r, b.rep_r) and torch.equal(a.rep_a, b.rep_a), "ring: r, a"
    assert not torch.equal(a.params.cpu(), _weights()[0]), "steps were applied"
    assert n_cur > 0, "some graphs came from the tick's own slot"
