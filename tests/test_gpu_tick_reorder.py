"""The fused tick's acting chain draws its coin, its pair forces and an exploring env's random
actions under and behind the forward (swarm_actk.h kDefer) instead of in the prologue.  Nothing it
computes may move: the fused tick stays bit-identical to the 3-launch tick (whose acting kernel
shares the body), the acting part stays on the oracle, and blocks with and without hand-off
graphs in one launch stay exact.
"""
import pytest
import torch

from oracle import swarm_oracle as O
from tests.conftest import assert_close_ulp
from tests.test_gpu_parity import Q_ULP, _assert_reward, _params, _rand_state, _tie_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sw():
    import swarm_amd
    swarm_amd.load_library()
    return swarm_amd


def _fused_equals_three_launch(sw, golden_weights, scen, N, B, slots, eps, ticks=6):
    """Every tick: ctrl, samples, grad, Q, actions, rewards; after flush(): params, target, moments,
    state.  Returns per tick the batch positions drawn from the slot the tick wrote (hand-offs)."""
    p = _params(golden_weights, "go_to" if scen == "GoTo" else "obstacle_avoidance", 2)
    kw = dict(seed=9, params=p, batch=B, eps=eps, update_target_every=2, replay_capacity=slots * B)
    a = sw.SwarmEngine(scen, N, B, **kw)
    b = sw.SwarmEngine(scen, N, B, **kw)
    assert a.fused
    a.reset(0)
    b.reset(0)
    handoffs = []
    for t in range(ticks):
        a.train_tick(full_out=True)
        b.train_tick3(full_out=True)
        torch.cuda.synchronize()
        ca, cb = a.read_ctrl(), b.read_ctrl()
        assert ca == cb, t
        assert torch.equal(a.samples, b.samples), t
        handoffs.append(((a.samples // B) == (ca["write_slot"] - 1) % slots).cpu())
        assert torch.equal(a.grad, b.grad), t
        assert torch.equal(a.q, b.q) and torch.equal(a.actions, b.actions) and torch.equal(a.reward, b.reward), t
    a.flush()
    b.flush()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.target, b.target)
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert torch.equal(a.state, b.state)
    assert a.handoff_errors() == 0
    return handoffs


# GoTo 8: 8 slots, one pair per lane (coin and pair geometry under the forward); OA 5: 8 slots,
# compacted forces (they keep their place, the coin moves); OA 12: 16 slots, nothing moves
@pytest.mark.parametrize("eps", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("scen,N,B", [("GoTo", 8, 16), ("ObstacleAvoidance", 5, 16), ("ObstacleAvoidance", 12, 8)])
def test_reordered_tick_equals_three_launch_tick(sw, golden_weights, scen, N, B, slots, eps):
    """B = S, rings of one and two slots: all or about half of the draws are hand-offs, so every TD
    block waits on acting waves of the same launch."""
    handoffs = _fused_equals_three_launch(sw, golden_weights, scen, N, B, slots, eps)
    if slots == 1:
        assert all(bool(h.all()) for h in handoffs)
    else:
        assert any(bool(h.any()) for h in handoffs)


@pytest.mark.parametrize("eps", [1.0, 0.0])
def test_reordered_acting_tick_against_oracle(sw, golden_weights, eps):
    """The fused tick's acting part at GoTo 8 x 16 against the oracle's act_tick, compared as
    test_act_tick_parity compares the acting kernel: eps = 1.0, every env takes the random
    actions drawn behind the forward; eps = 0.0, none does."""
    scen, N, B = "go_to", 8, 16
    p = _params(golden_weights, scen, 7)
    eng = sw.SwarmEngine(scen, N, B, seed=11, params=p, batch=B, eps=eps, replay_capacity=4 * B)
    assert eng.fused
    pos, vel = _rand_state(B, N, 21)
    eng.set_state(pos, vel)
    eng.ctrl[0] = 5   # tick
    eng.train_tick(full_out=True)
    torch.cuda.synchronize()
    ref = O.act_tick(O.unflatten_params(p), pos, vel, O.SCENARIO_GOTO, O.GRAPH_COMPLETE, 0, eps, 11, 5)
    assert bool(ref.explore.all()) if eps == 1.0 else not bool(ref.explore.any())
    assert_close_ulp(eng.q.cpu(), ref.q, Q_ULP, "Q", scale=1.0, rel_floor=1e-5)
    clear = _tie_mask(ref.q) | ref.explore[:, None]
    assert eps < 1.0 or bool(clear.all())
    assert torch.equal(eng.actions.cpu().long()[clear], ref.actions[clear])
    env = clear.all(-1)   # an env's step depends on its own agents' actions only
    assert bool(env.any())
    assert (eng.state.cpu()[..., :2] - ref.step["pos"])[env].abs().max() <= 1e-6
    if bool(env.all()):
        _assert_reward(eng.reward.cpu(), ref.step["rew"], scen, pos, ref.step["pos"])
    # replay push: slot 0 holds (s, a, r, s')
    assert torch.equal(eng.rep_s[0].cpu(), torch.cat([pos, vel], -1))
    assert torch.equal(eng.rep_a[0].cpu().long()[env], ref.actions[env])
    assert torch.equal(eng.rep_s1[0].cpu(), eng.state.cpu())
    assert eng.handoff_errors() == 0


def test_handoff_blocks_beside_ordinary_blocks(sw, golden_weights):
    """GoTo 8, B = S = 64, a ring of four slots: about a quarter of the draws are hand-offs, so one
    launch holds TD blocks (four graphs each) without a hand-off graph and blocks with some."""
    handoffs = _fused_equals_three_launch(sw, golden_weights, "GoTo", 8, 64, 4, 0.3)
    per_block = [h.view(-1, 4).sum(-1) for h in handoffs]
    assert any(bool((n == 0).any()) and bool((n > 0).any()) for n in per_block)
