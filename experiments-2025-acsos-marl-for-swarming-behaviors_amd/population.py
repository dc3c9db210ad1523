"""SwarmPopulation: P independent learners ticked together.

The reference runs its experiment once per seed (src/training/train_gcn_dqn.py:262-290: one
environment, batch 32, seeds 0-9 one after another).  At that shape a training tick is one acting
block and a few TD blocks, about 1 % of the chip, so the seeds can share the tick's two launches:

    swarm_pop_train_tick      grid (n_act + n_td, P): block (x, m) is block x of member m's
                              fused tick                                              (1 launch)
    swarm_pop_reduce_advance  grid (109, P): member m's slab sum, copy-back, ctrl     (1 launch)

All members share one configuration except the seed, and one set of optimizer
hyper-parameters.  Each member is an ordinary ``SwarmEngine`` (``pop.members[m]``: ``state_dict``,
``read_ctrl``, ``rollout``, ``flush`` ... work per member) that owns its state, replay ring,
learner, control block, slabs, hand-off workspace, samples and outputs; the population only moves
every member's control block, reward, avg_dist, hits and hand-off workspace into rows of
contiguous ``[P, ...]`` tensors, so the per-tick bookkeeping of a trainer is a fixed number of
launches whatever P is.  Members never exchange data: member m computes bit for bit what a lone
``SwarmEngine`` with its seed computes with ``train_tick`` (tests/test_gpu_population.py).
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch

from ._lib import CTRL, SwarmAdamCfg, SwarmConfig, SwarmPopMember, call, ptr
from .engine import SwarmEngine, capture_ticks, decode_ctrl, norm_flags


def _bytes_of(struct) -> bytes:
    return ctypes.string_at(ctypes.addressof(struct), ctypes.sizeof(struct))


def _copy_of(struct):
    return type(struct).from_buffer_copy(_bytes_of(struct))


class SwarmPopulation:
    def __init__(self, seeds: Sequence[int], **engine_kwargs):
        """``seeds`` plus the keyword arguments of ``SwarmEngine`` (everything but ``seed``)."""
        seeds = list(seeds)
        if not seeds:
            raise ValueError("a population needs at least one seed")
        if "seed" in engine_kwargs:
            raise ValueError("a population takes seeds=[...], not seed=")
        if not engine_kwargs.get("learn", True):
            raise ValueError("a population is made of learners: learn=False has nothing to tick together")
        if engine_kwargs.get("world_size", 1) > 1 or engine_kwargs.get("peer") is not None:
            raise ValueError("a population runs on one GPU: no world_size > 1, no peer exchange")
        self._adopt([SwarmEngine(seed=s, **engine_kwargs) for s in seeds])

    @classmethod
    def from_engines(cls, engines: Sequence[SwarmEngine]) -> "SwarmPopulation":
        """A population of engines that exist already (PopulationTrainer re-homes its trainers'
        engines this way).  They must agree in everything but the seed."""
        self = cls.__new__(cls)
        self._adopt(list(engines))
        return self

    # ------------------------------------------------------------------ construction
    def _adopt(self, members):
        if not members:
            raise ValueError("a population needs at least one member")
        first = members[0]
        self.lib = first.lib
        self.device = first.device

        def shared(e):   # what every member must share: the configuration without the seed, the optimizer
            c = _copy_of(e.cfg)
            c.seed = 0
            h = _copy_of(e.hp)
            h.flags = 0
            return _bytes_of(c), _bytes_of(h), e.capacity, e.device
        for e in members:
            if e.world_size > 1 or e.peer is not None:
                raise ValueError("a population runs on one GPU: no world_size > 1, no peer exchange")
            if not e.fused:
                raise ValueError("a population needs a configuration the fused training tick covers "
                                 "(a learner, n_agents <= 16, net='gcn', a complete, kNN or radius graph)")
            if shared(e) != shared(first):
                raise ValueError("the members of a population share one configuration (all but the seed) and one "
                                 "set of optimizer hyper-parameters")
        if len({id(e) for e in members}) != len(members):
            raise ValueError("an engine can be a member only once")
        self.members = members
        self.P = P = len(members)
        self.B, self.N = first.B, first.N
        self.cfg: SwarmConfig = _copy_of(first.cfg)      # cfg.seed is not used: each member's own is
        self.hp: SwarmAdamCfg = _copy_of(first.hp)
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # every member's control block, reward, avg_dist, hits and hand-off workspace as rows of
        # one tensor each; the members' attributes become views of their rows
        self.ctrl = torch.stack([e.ctrl for e in members])                      # [P, 32] int32
        self.reward = torch.stack([e.reward for e in members])                  # [P, B, N]
        self.avg_dist = torch.stack([e.avg_dist for e in members])              # [P, B]
        self.hits = torch.stack([e.hits for e in members])                      # [P, B]
        nb = first.tick_ws.numel()
        self.tick_ws = torch.zeros(P, -(-nb // 512) * 512, dtype=torch.uint8, device=dev)
        for m, e in enumerate(members):
            self.tick_ws[m, :nb].copy_(e.tick_ws)
            e.ctrl, e.reward, e.avg_dist, e.hits = self.ctrl[m], self.reward[m], self.avg_dist[m], self.hits[m]
            e.tick_ws = self.tick_ws[m, :nb]
            e.bind_outputs()
        # the descriptor tables in device memory, written once: one per output set of train_tick
        self._table_full = self._table(lambda e: e.out)
        self._table_min = self._table(lambda e: e.out_min)

    def _table(self, out_of) -> torch.Tensor:
        arr = (SwarmPopMember * self.P)()
        for m, e in enumerate(self.members):
            arr[m] = SwarmPopMember(e.cfg.seed, ptr(e.state), e.replay, e.learner, ptr(e.ctrl), out_of(e),
                                    ptr(e.slabs), ptr(e.tick_ws), ptr(e.samples))
        host = torch.frombuffer(bytearray(_bytes_of(arr)), dtype=torch.uint8)
        return host.to(self.device)

    # ------------------------------------------------------------------ the tick
    def train_tick(self, full_out: bool = False):
        """One fused training tick of every member: two launches.  Each member's TD batch indices
        go to its ``samples``; with full_out its Q, actions and obs are written too."""
        # the reduce's clip-norm partials describe every member's grad unless one declared a write
        dirty = any(e._grad_dirty for e in self.members)
        self.hp.flags = norm_flags(not dirty)
        table = self._table_full if full_out else self._table_min
        call(self.lib, "swarm_pop_train_tick", self.cfg, self.hp, ptr(table), self.P)
        if dirty:
            for e in self.members:
                e._grad_dirty = False   # the reduce below rewrites grad and its partials
        call(self.lib, "swarm_pop_reduce_advance", self.cfg, self.hp, ptr(table), self.P)

    def reset(self, episode=None):
        """Reset every member's environments (one small launch per member, once per episode)."""
        for e in self.members:
            e.reset(episode)

    def set_eps(self, eps):
        """Exploration epsilon of the next ticks: one value for all members, or one per member [P]."""
        col = self.ctrl.view(torch.float32)[:, CTRL["eps"]]
        if isinstance(eps, (int, float)):
            col.fill_(float(eps))
        else:
            e = torch.as_tensor(eps, dtype=torch.float32).reshape(-1)
            if e.numel() != self.P:
                raise ValueError(f"set_eps: {e.numel()} values for {self.P} members")
            col.copy_(e.to(self.device))

    def flush(self):
        """Apply every member's pending optimizer step (one small launch per member)."""
        for e in self.members:
            e.flush()

    def capture(self, n_ticks: int, fn=None):
        """Capture n_ticks calls of ``fn`` (default train_tick) into one hipGraph, on one stream."""
        return capture_ticks(self.device, n_ticks, fn or self.train_tick)

    # ------------------------------------------------------------------ reading back
    def handoff_errors(self) -> list:
        """Every member's count of hand-off waits that hit their bound (all 0 in a correct run);
        one device read."""
        return self.tick_ws[:, :4].contiguous().view(torch.int32).reshape(-1).tolist()

    def check_handoffs(self):
        """Raise if any member's fused tick had a hand-off wait overrun (SwarmEngine.check_handoffs)."""
        bad = {m: n for m, n in enumerate(self.handoff_errors()) if n}
        if bad:
            raise RuntimeError(f"population tick: hand-off wait(s) overran their bound (member: count) {bad}; the "
                               "graphs they waited for were dropped from their TD batches")

    def read_ctrl(self) -> list:
        """Every member's control block as SwarmEngine.read_ctrl gives it; one device read."""
        c = self.ctrl.cpu()
        return [decode_ctrl(c[m]) for m in range(self.P)]
