"""The learning prologue's LDS weight image (swarm_adam.h WImageSlots, store_w_lds).

Every block of a training tick applies the pending optimizer step in registers and writes the
weights into its padded LDS image; the slots are formed from the thread index while the step's
operands are in flight (swarm_common.h lds_index_flat).  A parameter in a wrong slot shows in the
forward: the tick's Q against swarm_q_forward (whose kernel stages the flat vector itself) on the
acting side, the tick's gradient against the unfused TD kernel on the TD side.  Everything is
compared bit for bit.

Shapes: 5 envs (the second acting block has one live wave), N = 5, 8 (8-slot kernels) and 12
(16-slot), GAT and GCN, a batch of 4 graphs and a replay ring of two slots (hand-off blocks exist).
"""
import pytest
import torch

from oracle import swarm_oracle as O
from tests.test_gpu_parity import _params, _rand_state

pytestmark = pytest.mark.gpu

B, S, SLOTS = 5, 4, 2
CASES = [(N, conv) for N in (5, 8, 12) for conv in ("gat", "gcn")]


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _engine(sw, N, conv, params, every=3):
    eng = sw.SwarmEngine("GoTo", N, B, seed=13, params=params, batch=S, eps=0.3, update_target_every=every,
                         replay_capacity=SLOTS * B, conv=conv)
    assert eng.fused
    pos, vel = _rand_state(B, N, 40 + N)
    eng.set_state(pos, vel)
    return eng


def _q_forward(sw, eng, params, state):
    """swarm_q_forward of `params` on the node features of `state` [B, N, 4]"""
    from swarm_amd._lib import call, ptr
    st = state.cpu()
    x = O.node_features(st[..., :2], st[..., 2:]).reshape(B * eng.N, 7).contiguous().cuda()
    p = params.detach().clone().contiguous()
    q = torch.zeros(B * eng.N, 9, device="cuda")
    call(eng.lib, "swarm_q_forward", eng.cfg, ptr(p), ptr(x), None, ptr(q))
    torch.cuda.synchronize()
    return q.view(B, eng.N, 9)


def _distinct_weights():
    """1,673 distinct values in +-0.21, not monotone in the parameter index"""
    n = 1673
    p = (((torch.arange(n, dtype=torch.int64) * 7919) % n) - n // 2).to(torch.float32) / 4096.0
    assert p.unique().numel() == n
    return p


@pytest.mark.parametrize("N,conv", CASES)
def test_no_pending_step_stages_every_parameter(sw, N, conv):
    """trained = 0: the image is w_cur.  Acting side: the tick's Q == swarm_q_forward; TD side: the
    tick's gradient == swarm_td_grad + swarm_grad_reduce on the same batch."""
    from swarm_amd._lib import N_PARAMS
    p = _distinct_weights()
    a, b = _engine(sw, N, conv, p), _engine(sw, N, conv, p)
    s0 = a.state.clone()
    assert a.read_ctrl()["trained"] == 0
    a.train_tick(full_out=True)
    torch.cuda.synchronize()
    assert a.handoff_errors() == 0
    assert torch.equal(a.q, _q_forward(sw, a, a.params, s0))
    assert torch.equal(a.params.cpu(), p) and torch.equal(a.w_nxt.cpu(), p)
    # the unfused kernels on the transitions the same tick pushes
    b.act(push=True)
    torch.cuda.synchronize()
    assert torch.equal(a.q, b.q) and torch.equal(a.rep_s1, b.rep_s1) and torch.equal(a.rep_a, b.rep_a)
    b._td(b.params, a.samples.clone(), None)
    b.launch_grad_reduce()
    torch.cuda.synchronize()
    assert float(b.grad[:N_PARAMS].abs().max()) > 0.0
    assert torch.equal(a.grad[:N_PARAMS + 1], b.grad[:N_PARAMS + 1])


@pytest.mark.parametrize("partials", [True, False])
@pytest.mark.parametrize("every", [1, 3])   # the pending step's tick is 1: a target-sync tick, or none
@pytest.mark.parametrize("N,conv", CASES)
def test_pending_step_reaches_the_image(sw, golden_weights, N, conv, every, partials):
    """The second tick applies the first's gradient.  Weights, moments and target == the 3-launch
    tick's and swarm_adam_step's; the forward ran on the stepped weights (Q == swarm_q_forward on
    w_nxt); the gradient (TD blocks' online and target images) == the 3-launch tick's."""
    from swarm_amd._lib import ADAM_F_NORM_PARTIALS, CTRL
    p = _params(golden_weights, "go_to", 2)
    a, b, c = (_engine(sw, N, conv, p, every) for _ in range(3))
    a.train_tick(full_out=True)
    b.train_tick3(full_out=True)
    torch.cuda.synchronize()
    assert a.read_ctrl() == b.read_ctrl() and a.read_ctrl()["trained"] == 1 and a.read_ctrl()["tick"] == 1
    assert torch.equal(a.grad, b.grad) and float(a.grad[:1673].abs().max()) > 0.0
    # swarm_adam_step on the same operands: it takes the step of tick ctrl.tick and advances
    c.grad.copy_(a.grad)
    c.ctrl.copy_(a.ctrl)
    c.ctrl[CTRL["tick"]] -= 1
    c.adam()
    s1 = a.state.clone()
    if not partials:   # the prologue forms the clip norm from the gradient itself
        a.grad_written()
        b.grad_written()
    a.train_tick(full_out=True)
    b.train_tick3(full_out=True)
    torch.cuda.synchronize()
    assert a.hp.flags == (ADAM_F_NORM_PARTIALS if partials else 0)
    assert a.handoff_errors() == 0
    assert a.read_ctrl() == b.read_ctrl() and a.read_ctrl()["adam_step"] == 1
    assert a.read_ctrl()["grad_norm"] == c.read_ctrl()["grad_norm"]
    for x, y, z in ((a.params, b.params, c.params), (a.adam_m, b.adam_m, c.adam_m), (a.adam_v, b.adam_v, c.adam_v),
                    (a.target, b.target, c.target)):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert not torch.equal(a.params.cpu(), p)
    assert torch.equal(a.target, a.params) if every == 1 else torch.equal(a.target.cpu(), p)
    assert torch.equal(a.w_nxt, a.params)
    assert torch.equal(a.q, _q_forward(sw, a, a.w_nxt, s1))
    assert torch.equal(a.q, b.q) and torch.equal(a.actions, b.actions) and torch.equal(a.samples, b.samples)
    assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("N,conv", CASES)
def test_held_rank_keeps_the_current_weights(sw, golden_weights, N, conv):
    """ctrl.peer_hold set: the pending step is not applied and the image is w_cur."""
    from swarm_amd._lib import CTRL
    p = _params(golden_weights, "go_to", 2)
    a, b = _engine(sw, N, conv, p, 1), _engine(sw, N, conv, p, 1)
    a.train_tick(full_out=True)
    b.train_tick3(full_out=True)
    torch.cuda.synchronize()
    assert a.read_ctrl()["trained"] == 1 and float(a.grad[:1673].abs().max()) > 0.0
    for e in (a, b):
        e.ctrl[CTRL["peer_hold"]] = 1
    s1 = a.state.clone()
    a.train_tick(full_out=True)
    b.train_tick3(full_out=True)
    torch.cuda.synchronize()
    assert a.handoff_errors() == 0
    assert a.read_ctrl() == b.read_ctrl() and a.read_ctrl()["adam_step"] == 0
    for x, y in ((a.params, b.params), (a.adam_m, b.adam_m), (a.adam_v, b.adam_v), (a.target, b.target)):
        assert torch.equal(x, y)
    assert torch.equal(a.params.cpu(), p) and torch.equal(a.target.cpu(), p) and torch.equal(a.w_nxt.cpu(), p)
    assert float(a.adam_m.abs().max()) == 0.0 and float(a.adam_v.abs().max()) == 0.0
    assert torch.equal(a.q, _q_forward(sw, a, a.params, s1))
    assert torch.equal(a.q, b.q) and torch.equal(a.grad, b.grad)
