"""SwarmPopulation: P independent learners ticked together.

The reference runs its experiment once per seed (src/training/train_gcn_dqn.py:262-290: one
environment, batch 32, seeds 0-9 one after another).  At that shape a training tick is one acting
block and a few TD blocks, about 1 % of the chip, so the seeds can share the tick's two launches:

    swarm_pop_train_tick      grid (n_act + n_td, P): block (x, m) is block x of member m's
                              fused tick                                              (1 launch)
    swarm_pop_reduce_advance  grid (109, P): member m's slab sum, copy-back, ctrl     (1 launch)

All members share one configuration except the seed.  The optimizer's hyper-parameters (lr,
gamma, betas, adam_eps, max_norm, update_target_every) may be one value for all or one per
member: a sweep runs in the same two launches (swarm_pop_train_tick_hp /
swarm_pop_reduce_advance_hp read member m's row of a device table; ``per_member_hp``).  Each
member is an ordinary ``SwarmEngine`` (``pop.members[m]``: ``state_dict``, ``read_ctrl``,
``rollout``, ``flush`` ... work per member) that owns its state, replay ring,
learner, control block, slabs, hand-off workspace, samples and outputs; the population only moves
every member's control block, reward, avg_dist, hits and hand-off workspace into rows of
contiguous ``[P, ...]`` tensors, so the per-tick bookkeeping of a trainer is a fixed number of
launches whatever P is.  Members never exchange data: member m computes bit for bit what a lone
``SwarmEngine`` with its seed computes with ``train_tick`` (tests/test_gpu_population.py).

Evaluation has the same shape (1-8 environments per policy, one or two blocks per rollout launch):
``ActorPopulation`` rolls out P existing engines in one swarm_pop_rollout launch, grid
(ceil(B / 4), P), and ``SwarmPopulation.evaluate`` runs every member's current weights on one set
of evaluation environments that way (tests/test_gpu_pop_rollout.py).

Population-based training closes the loop on the device: ``SwarmPopulation.exploit(score, ...)``
(swarm_pop_exploit) ranks the members by a device score, copies the best members' learners,
optimizer state and hyper-parameter rows over the worst and perturbs the copies' lr / gamma, in two
launches with no host round trip (tests/test_gpu_pop_pbt.py).

The three-layer GAT (``net="gat3"``, the Flocking checkpoints' network) has a population of its own:
``SwarmGat3Population`` ticks P ``SwarmGat3Engine`` learners in the four launches of that engine's
unfused tick (swarm_pop_gat3_act_step / _td_grad / _adam_step, the member as the grid's second
dimension), with the same per-member hyper-parameters, capture and evaluation, and without
population-based training (tests/test_gpu_gat3_population.py).
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence

import torch

from . import _lib
from ._lib import (CTRL, SwarmActOut, SwarmAdamCfg, SwarmConfig, SwarmGat3Member, SwarmPopActor, SwarmPopMember, call,
                   ptr, size)
from .engine import (CONVS, GRAPHS, HP_FIELDS, NETS, SwarmEngine, SwarmGat3Engine, capture_ticks, check_hp_values,
                     decode_ctrl, norm_flags)


def _bytes_of(struct) -> bytes:
    return ctypes.string_at(ctypes.addressof(struct), ctypes.sizeof(struct))


def _copy_of(struct):
    return type(struct).from_buffer_copy(_bytes_of(struct))


def _is_pair(v) -> bool:
    return isinstance(v, (tuple, list)) and len(v) == 2 and not any(hasattr(b, "__len__") for b in v)


def member_hp_kwargs(P: int, engine_kwargs: dict) -> list:
    """Split SwarmPopulation's keyword arguments into one dict per member, with nothing built: each
    of lr, gamma, adam_eps, max_norm and update_target_every is one value for all members or a
    sequence of P values; betas is the shared pair (a bare 2-sequence of numbers always is) or a
    sequence of P pairs.  Raises ValueError for a sequence of another length and for a value
    ``check_hp_values`` refuses (update_target_every < 1, a non-finite number ...)."""
    per_member = [dict(engine_kwargs) for _ in range(P)]
    for k in HP_FIELDS:
        if k not in engine_kwargs:
            continue
        v = engine_kwargs[k]
        if hasattr(v, "tolist"):   # a numpy array or a tensor of values
            v = v.tolist()
        seq = isinstance(v, (tuple, list)) and not (k == "betas" and _is_pair(v))
        if seq and len(v) != P:
            raise ValueError(f"{k}: {len(v)} values for {P} members")
        for m, kw in enumerate(per_member):
            kw[k] = v[m] if seq else v
            if k == "betas" and isinstance(kw[k], list):
                kw[k] = tuple(kw[k])
            check_hp_values(**{k: kw[k]})
    return per_member


def _take_row(hp: SwarmAdamCfg, row: SwarmAdamCfg):
    """what a member's row decides (take_member_hp, csrc/swarm_popk.h): hp keeps its batch,
    world_size and flags"""
    for k in ("lr", "beta1", "beta2", "eps", "max_norm", "gamma", "update_target_every", "lr_d", "beta1_d", "beta2_d"):
        setattr(hp, k, getattr(row, k))


PBT_FIELDS = {"lr": _lib.PBT_F_LR, "gamma": _lib.PBT_F_GAMMA}


def pbt_round_cfg(P: int, score, device, *, round: int, seed: int = 0, frac: float = 0.25, perturb=(0.8, 1.2),
                  fields=("lr",), lr_bounds=(1e-6, 1e-1), gamma_bounds=(0.0, 0.9999)) -> _lib.SwarmPbtCfg:
    """``SwarmPopulation.exploit``'s arguments checked (ValueError; nothing is launched) and packed
    into the swarm_pbt_cfg of one round for a population of P members on ``device``."""
    if P > _lib.PBT_MAX_MEMBERS:
        raise ValueError(f"exploit: {P} members, at most {_lib.PBT_MAX_MEMBERS}")
    if not (isinstance(score, torch.Tensor) and score.dtype == torch.float32 and tuple(score.shape) == (P,)
            and score.device == torch.device(device) and score.is_contiguous()):
        raise ValueError(f"score: a contiguous float32 tensor of shape [{P}] on {device}")
    if isinstance(round, bool) or not isinstance(round, int) or not 0 <= round < 1 << 32:
        raise ValueError(f"round must be an integer in [0, 2^32), not {round!r}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, not {seed!r}")
    if not _is_real(frac) or not 0.0 <= frac <= 0.5:
        raise ValueError(f"frac must lie in [0, 0.5] (parents and children are disjoint sets), not {frac!r}")
    if isinstance(fields, str):
        fields = (fields,)
    unknown = [f for f in fields if f not in PBT_FIELDS]
    if unknown:
        raise ValueError(f"fields: {unknown!r} cannot be perturbed ({', '.join(PBT_FIELDS)})")
    for name, pair, low_ok in (("perturb", perturb, False), ("lr_bounds", lr_bounds, False),
                               ("gamma_bounds", gamma_bounds, True)):
        if not (_is_pair(pair) and all(_is_real(v) for v in pair)):
            raise ValueError(f"{name} must be a pair of finite numbers, not {pair!r}")
        if not pair[0] <= pair[1] or not (low_ok or pair[0] > 0):
            raise ValueError(f"{name} must be in order{'' if low_ok else ' and > 0'}, not {pair!r}")
    bits = 0
    for f in fields:
        bits |= PBT_FIELDS[f]
    pbt = _lib.SwarmPbtCfg(seed & 0xFFFFFFFFFFFFFFFF, round, int(frac * P), bits, perturb[0], perturb[1],
                           gamma_bounds[0], gamma_bounds[1], float(lr_bounds[0]), float(lr_bounds[1]))
    if not (pbt.perturb_lo > 0 and math.isfinite(pbt.perturb_hi)):   # as rounded to fp32
        raise ValueError(f"perturb must be a pair of finite fp32 numbers > 0, not {perturb!r}")
    return pbt


def _is_real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


class _Population:
    """What ``SwarmPopulation`` (the one-layer network's fused tick) and ``SwarmGat3Population`` (the
    three-layer network's unfused tick) share: members that are ordinary engines of ``member_class``
    with one configuration, their control blocks and trainer outputs as rows of [P, ...] tensors, the
    descriptor tables and the optimizer row table in device memory, and everything that needs no
    more than those.  A subclass gives ``member_class``, ``_check_member``, ``_table`` and
    ``train_tick``, and may re-home more buffers (``_rehome_more``)."""
    member_class = SwarmEngine

    def __init__(self, seeds: Sequence[int], **engine_kwargs):
        """``seeds`` plus the keyword arguments of the member engine (everything but ``seed``); the
        optimizer's (``engine.HP_FIELDS``) may each be a sequence of one value per member
        (``member_hp_kwargs``)."""
        seeds = list(seeds)
        if not seeds:
            raise ValueError("a population needs at least one seed")
        if "seed" in engine_kwargs:
            raise ValueError("a population takes seeds=[...], not seed=")
        if not engine_kwargs.get("learn", True):
            raise ValueError("a population is made of learners: learn=False has nothing to tick together")
        if engine_kwargs.get("world_size", 1) > 1 or engine_kwargs.get("peer") is not None:
            raise ValueError("a population runs on one GPU: no world_size > 1, no peer exchange")
        per_member = member_hp_kwargs(len(seeds), engine_kwargs)
        self._adopt([self.member_class(seed=s, **kw) for s, kw in zip(seeds, per_member)])

    @classmethod
    def from_engines(cls, engines: Sequence[SwarmEngine]):
        """A population of engines that exist already (a population trainer re-homes its trainers'
        engines this way).  They must agree in everything but the seed and the optimizer's
        per-member hyper-parameters: one configuration, batch, ring capacity and device."""
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

        def shared(e):   # what every member must share: the configuration without the seed, and what
            c = _copy_of(e.cfg)   # of the optimizer fixes the launch (batch: grid, S, loss scale, slabs)
            c.seed = 0
            return _bytes_of(c), e.hp.batch, e.hp.world_size, e.capacity, e.device
        for e in members:
            if e.world_size > 1 or e.peer is not None:
                raise ValueError("a population runs on one GPU: no world_size > 1, no peer exchange")
            self._check_member(e)
            if shared(e) != shared(first):
                raise ValueError("the members of a population share one configuration (all but the seed), one "
                                 "batch size and one ring capacity")
        if len({id(e) for e in members}) != len(members):
            raise ValueError("an engine can be a member only once")
        self.members = members
        self.P = P = len(members)
        self.B, self.N = first.B, first.N
        self.cfg: SwarmConfig = _copy_of(first.cfg)      # cfg.seed is not used: each member's own is
        # the shared hp: batch, world_size and the launch's flags for every member; its other
        # fields are the optimizer of every member while per_member_hp is False
        self.hp: SwarmAdamCfg = _copy_of(first.hp)
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # every member's control block, reward, avg_dist and hits (and what _rehome_more adds) as
        # rows of one tensor each; the members' attributes become views of their rows
        self.ctrl = torch.stack([e.ctrl for e in members])                      # [P, 32] int32
        self.reward = torch.stack([e.reward for e in members])                  # [P, B, N]
        self.avg_dist = torch.stack([e.avg_dist for e in members])              # [P, B]
        self.hits = torch.stack([e.hits for e in members])                      # [P, B]
        for m, e in enumerate(members):
            e.ctrl, e.reward, e.avg_dist, e.hits = self.ctrl[m], self.reward[m], self.avg_dist[m], self.hits[m]
        self._rehome_more()
        for e in members:
            e.bind_outputs()
        # the descriptor tables in device memory, written once: one per output set of train_tick
        self._table_full = self._table(lambda e: e.out)
        self._table_min = self._table(lambda e: e.out_min)
        # every member's optimizer row (its engine's hp) in device memory, read by the _hp entry
        # points on every launch; rewritten by set_member_hp
        rows = (SwarmAdamCfg * P)(*[self._row(e) for e in members])
        self._hp_table = torch.frombuffer(bytearray(_bytes_of(rows)), dtype=torch.uint8).to(dev).view(P, -1)
        self.per_member_hp = self._rows_differ()
        self._evals = {}   # evaluate(): (n_envs, graph, knn_k) -> its launches, start and state rows
        # exploit(): each member's parent of the last PBT round; the device table's rows are ahead
        # of the members' host hp after an exploit(sync=False), until sync_hp()
        self.parent = torch.arange(P, dtype=torch.int32, device=dev)
        self._hp_stale = False

    def _check_member(self, e):
        """raise ValueError unless engine e can be a member"""
        raise NotImplementedError

    def _rehome_more(self):
        """re-home what the subclass's tick needs besides ctrl, reward, avg_dist and hits"""

    @staticmethod
    def _row(e) -> SwarmAdamCfg:
        r = _copy_of(e.hp)
        r.flags = 0   # a row's batch, world_size and flags are ignored; flags change per launch
        return r

    def _rows_differ(self) -> bool:
        return len({_bytes_of(self._row(e)) for e in self.members}) > 1

    def set_member_hp(self, m: int, **fields):
        """Change member m's optimizer hyper-parameters (``engine.HP_FIELDS``) for the ticks that
        follow: ``members[m].set_hp(**fields)`` (so the member's own ``flush`` agrees) plus row m of
        the device table, and ``per_member_hp`` becomes True if the rows now differ.  It means what
        ``SwarmEngine.set_hp`` between two eager ticks means for a lone engine, bit for bit (a new
        lr acts one optimizer step later, see there).  The table is read on every launch, so a
        hipGraph captured while ``per_member_hp`` was True sees the new row at its next replay; one
        captured while it was False holds the shared hp as a kernel argument and does not (set
        ``per_member_hp = True`` before capturing a population whose rows will change)."""
        if not 0 <= m < self.P:
            raise ValueError(f"member {m} of {self.P}")
        if self._hp_stale:   # the row is rewritten whole from the member's host hp
            self.sync_hp()
        e = self.members[m]
        e.set_hp(**fields)   # validates
        row = torch.frombuffer(bytearray(_bytes_of(self._row(e))), dtype=torch.uint8)
        self._hp_table[m].copy_(row)   # on the current stream: behind every tick issued so far
        if m == 0:   # the shared hp follows member 0, as at adoption (all there is when the rows are equal)
            flags = self.hp.flags
            self.hp = _copy_of(e.hp)
            self.hp.flags = flags
        self.per_member_hp = self.per_member_hp or self._rows_differ()

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

    def capture(self, n_ticks: int, fn=None):
        """Capture n_ticks calls of ``fn`` (default train_tick) into one hipGraph, on one stream."""
        return capture_ticks(self.device, n_ticks, fn or self.train_tick)

    # ------------------------------------------------------------------ reading back
    def read_ctrl(self) -> list:
        """Every member's control block as SwarmEngine.read_ctrl gives it; one device read."""
        c = self.ctrl.cpu()
        return [decode_ctrl(c[m]) for m in range(self.P)]

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, n_envs: int, n_ticks: int, *, seed: int, episode: int = 0, graph=None, knn_k=None,
                 eps: float = 0.0):
        """A rollout (greedy while ``eps`` is 0) of every member's current weights on ``n_envs``
        evaluation environments, the same for every member: one reset keyed (``seed``,
        ``episode``) whose start is copied to every member's row of an evaluation state buffer,
        then one swarm_pop_rollout launch.  ``graph`` / ``knn_k``: the evaluation graph (default the
        training graph's).  Returns ``ActorPopulation.rollout``'s dict ([P, ...] device tensors,
        the population's own buffers: the next evaluation of the same shape overwrites them).

        It reads ``members[m].params`` as they stand, with no ``flush``: after a tick's two
        launches that row holds the weights the tick acted with, and a pending optimizer step
        stays pending.  It writes only its own state and output buffers (built once per shape), so
        the training run keeps every bit: control blocks, replay rings, env states, Philox streams.
        Row m equals ``evaluation_engine(members[m].cfg, ...)``'s lone reset + rollout."""
        key = (n_envs, graph, knn_k)
        ev = self._evals.get(key)
        if ev is None:
            cfg = evaluation_config(self.cfg, n_envs, graph, knn_k)
            nst = max(size(self.lib, "swarm_state_floats", cfg), 1)
            ev = self._evals[key] = (_PopRollout(self.lib, self.device, cfg, self.P),
                                     torch.zeros(nst, dtype=torch.float32, device=self.device),
                                     torch.zeros(self.P, nst, dtype=torch.float32, device=self.device))
        roll, start, states = ev
        roll.cfg.seed = seed & 0xFFFFFFFFFFFFFFFF
        call(self.lib, "swarm_env_reset", roll.cfg, ptr(start), episode)
        states.copy_(start.expand_as(states))
        res = roll.prepare(n_ticks, [roll.cfg.seed] * self.P, [ptr(e.params) for e in self.members],
                           [ptr(states[m]) for m in range(self.P)], 0, eps, False)
        roll.launch(n_ticks)
        return res


class SwarmPopulation(_Population):
    """P independent learners of the one-layer network ticked together by the fused tick (the module
    docstring): two launches per tick, population-based training on the device."""
    member_class = SwarmEngine

    def _check_member(self, e):
        if not e.fused:
            raise ValueError("a population needs a configuration the fused training tick covers "
                             "(a learner, n_agents <= 16, net='gcn', a complete, kNN or radius graph); "
                             "SwarmGat3Engine learners (net='gat3') form a SwarmGat3Population")

    def _rehome_more(self):
        """every member's hand-off workspace as a row of one tensor"""
        nb = self.members[0].tick_ws.numel()
        self.tick_ws = torch.zeros(self.P, -(-nb // 512) * 512, dtype=torch.uint8, device=self.device)
        for m, e in enumerate(self.members):
            self.tick_ws[m, :nb].copy_(e.tick_ws)
            e.tick_ws = self.tick_ws[m, :nb]

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
        go to its ``samples``; with full_out its Q, actions and obs are written too.

        While ``per_member_hp`` is False (all rows equal) these are swarm_pop_train_tick and
        swarm_pop_reduce_advance with the shared hp as a kernel argument; otherwise the _hp pair,
        which reads each member's row of the device table."""
        # the reduce's clip-norm partials describe every member's grad unless one declared a write
        dirty = any(e._grad_dirty for e in self.members)
        self.hp.flags = norm_flags(not dirty)
        table = self._table_full if full_out else self._table_min
        hp_table = (ptr(self._hp_table),) if self.per_member_hp else ()
        sfx = "_hp" if self.per_member_hp else ""
        call(self.lib, "swarm_pop_train_tick" + sfx, self.cfg, self.hp, *hp_table, ptr(table), self.P)
        if dirty:
            for e in self.members:
                e._grad_dirty = False   # the reduce below rewrites grad and its partials
        call(self.lib, "swarm_pop_reduce_advance" + sfx, self.cfg, self.hp, *hp_table, ptr(table), self.P)

    # ------------------------------------------------------------------ population-based training
    def exploit(self, score, *, round: int, seed: int = 0, frac: float = 0.25, perturb=(0.8, 1.2), fields=("lr",),
                lr_bounds=(1e-6, 1e-1), gamma_bounds=(0.0, 0.9999), sync: bool = True):
        """One round of population-based training on the device (swarm_pop_exploit: two launches, no
        host round trip).  ``score`` is a [P] float32 tensor on the population's device, higher is
        better (NaN is worst).  The ``n_replace = int(frac * P)`` worst members (0 <= frac <= 0.5)
        each take over one of the n_replace best: the seven learner rows, the gradient with a
        pending step, the optimizer's control words and the hyper-parameter row; then the child's
        ``fields`` ("lr", "gamma") are multiplied by one of the two ``perturb`` factors (gamma as
        1 - (1 - gamma) * f) and clamped to their bounds.  A child keeps its own tick, ring, env
        state, eps and Philox streams; parents and the members in between are not written.  The
        draws are Philox blocks keyed (``seed``, ``round``, member): a round is reproducible, and a
        new ``round`` draws anew.  Returns ``parent``, a device int32 [P] (the population's own
        buffer; parent[m] == m for every member that was not replaced).

        It sets ``per_member_hp = True`` before the call: the children's rows now differ.  The
        table is read on every launch, so a hipGraph captured while ``per_member_hp`` was True sees
        the new rows at its next replay; one captured while it was False holds the shared hp as a
        kernel argument and does not (set ``per_member_hp = True`` before capturing a population
        that will be exploited).  ``round`` is a kernel argument: a captured exploit replays the
        same round.

        ``sync=True`` ends with ``sync_hp()`` (one device read).  With ``sync=False`` nothing is
        read back (the call can be captured) and the members' host ``hp`` lag behind the device
        rows until ``sync_hp()``; ``flush`` and ``set_member_hp`` call it first when needed.
        Arguments are checked (ValueError) before anything is launched."""
        pbt = pbt_round_cfg(self.P, score, self.device, round=round, seed=seed, frac=frac, perturb=perturb,
                            fields=fields, lr_bounds=lr_bounds, gamma_bounds=gamma_bounds)
        self.per_member_hp = True
        call(self.lib, "swarm_pop_exploit", pbt, ptr(score), ptr(self._hp_table), ptr(self._table_min), self.P,
             ptr(self.parent))
        self._hp_stale = pbt.n_replace > 0
        if sync:
            self.sync_hp()
        return self.parent

    def sync_hp(self):
        """Bring every ``members[m].hp`` and the shared ``hp`` (which follows member 0) in line with
        the device row table: one device read.  Each keeps its own batch, world_size and flags
        (a row's are ignored by the kernels).  Needed after ``exploit(sync=False)`` before a
        member's host hp is passed to the library (a member's own ``flush``)."""
        rows = self._hp_table.cpu().numpy().tobytes()
        n = ctypes.sizeof(SwarmAdamCfg)
        for m, e in enumerate(self.members):
            _take_row(e.hp, SwarmAdamCfg.from_buffer_copy(rows[m * n:(m + 1) * n]))
        _take_row(self.hp, self.members[0].hp)
        self._hp_stale = False

    def flush(self):
        """Apply every member's pending optimizer step (one small launch per member)."""
        if self._hp_stale:   # swarm_adam_flush takes each member's host hp
            self.sync_hp()
        for e in self.members:
            e.flush()

    # ------------------------------------------------------------------ hand-offs
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


class SwarmGat3Population(_Population):
    """P independent learners of the three-layer GAT (``SwarmGat3Engine``s, ``net="gat3"``: the
    reference's Flocking experiment, ten seeds of one environment each) ticked together: the four
    launches of ``SwarmGat3Engine.train_tick``, each once for all members,

        swarm_pop_gat3_act_step   grid (ceil(B / 4), P)                                     (1 launch)
        swarm_pop_gat3_td_grad    grid (TD blocks of the batch, P), then the slab sum (26, P) (2 launches)
        swarm_pop_gat3_adam_step  grid (1, P)                                               (1 launch)

    ``SwarmGat3Population(seeds=[...], **kw)`` takes ``SwarmGat3Engine``'s keyword arguments, the
    optimizer's one value for all or one per member; ``from_engines`` adopts existing engines.
    ``pop.members[m]`` stays an ordinary ``SwarmGat3Engine``.  Member m computes bit for bit what a
    lone ``SwarmGat3Engine`` with its seed computes with ``train_tick``
    (tests/test_gpu_gat3_population.py).  ``set_member_hp``, ``per_member_hp``, ``reset``,
    ``set_eps``, ``capture``, ``read_ctrl`` and ``evaluate`` are ``SwarmPopulation``'s.  The optimizer
    step is applied at once, so ``flush`` does nothing; there is no population-based training and
    no hand-off (``exploit``, ``handoff_errors``, ``check_handoffs`` raise ValueError)."""
    member_class = SwarmGat3Engine

    def _check_member(self, e):
        if not isinstance(e, SwarmGat3Engine):
            raise ValueError("a SwarmGat3Population is made of SwarmGat3Engine learners (net='gat3'); SwarmEngine "
                             "learners form a SwarmPopulation")

    def _table(self, out_of) -> torch.Tensor:
        arr = (SwarmGat3Member * self.P)()
        for m, e in enumerate(self.members):
            arr[m] = SwarmGat3Member(e.cfg.seed, ptr(e.state), e.replay, ptr(e.params), ptr(e.target), ptr(e.adam_m),
                                     ptr(e.adam_v), ptr(e.grad), ptr(e.ctrl), out_of(e), ptr(e.slabs), ptr(e.samples))
        host = torch.frombuffer(bytearray(_bytes_of(arr)), dtype=torch.uint8)
        return host.to(self.device)

    def train_tick(self, full_out: bool = False):
        """One training tick of every member: four launches.  Each member's TD batch indices go to
        its ``samples``; with full_out its Q, actions and obs are written too.

        While ``per_member_hp`` is False (all rows equal) the shared hp is a kernel argument;
        otherwise the TD and optimizer launches read each member's row of the device table."""
        table = ptr(self._table_full if full_out else self._table_min)
        hp_table = ptr(self._hp_table) if self.per_member_hp else None
        call(self.lib, "swarm_pop_gat3_act_step", self.cfg, table, self.P)
        call(self.lib, "swarm_pop_gat3_td_grad", self.cfg, self.hp, hp_table, table, self.P)
        call(self.lib, "swarm_pop_gat3_adam_step", self.cfg, self.hp, hp_table, table, self.P)

    def flush(self):
        """Nothing is ever pending: every tick applies its optimizer step at once."""

    def exploit(self, *args, **kw):
        raise ValueError("SwarmGat3Population has no population-based training: swarm_pop_exploit works on "
                         "swarm_pop_member tables (the one-layer network's SwarmPopulation)")

    def _no_handoff(self, *args, **kw):
        raise ValueError("SwarmGat3Population ticks unfused (act, TD gradient, optimizer step): there is no fused "
                         "tick and so no hand-off to count")

    handoff_errors = check_handoffs = _no_handoff


def evaluation_config(cfg: SwarmConfig, n_envs: int, graph=None, knn_k=None) -> SwarmConfig:
    """The configuration a learner of ``cfg`` is evaluated with: ``n_envs`` environments that each
    draw their own start (no shared reset centre), the graph ``graph`` / ``knn_k`` (names of
    ``engine.GRAPHS``; default ``cfg``'s own), everything else as trained."""
    c = _copy_of(cfg)
    c.n_envs, c.env_offset = n_envs, 0
    c.flags &= ~_lib.F_SHARED_RESET
    if graph is not None:
        c.graph = GRAPHS[graph]
    if knn_k is not None:
        c.knn_k = knn_k
    return c


def evaluation_engine(cfg: SwarmConfig, n_envs: int, seed: int, graph=None, knn_k=None) -> SwarmEngine:
    """A lone acting engine of ``evaluation_config`` (a lone trainer's evaluation; the reference
    side of ``SwarmPopulation.evaluate``)."""
    c = evaluation_config(cfg, n_envs, graph, knn_k)
    names = lambda table, v: next(k for k, x in table.items() if x == v)   # noqa: E731
    return SwarmEngine(c.scenario, c.n_agents, n_envs, seed=seed, graph=names(GRAPHS, c.graph), knn_k=c.knn_k,
                       conv=names(CONVS, c.conv), radius=c.radius, learn=False, shared_reset=False,
                       random_oa=bool(c.flags & _lib.F_RANDOM_OA), eps=0.0, net=names(NETS, c.net),
                       params=torch.zeros(_lib.GAT3_N_PARAMS if c.net == _lib.NET_GAT3 else _lib.N_PARAMS))


def _per_actor(v, P: int, name: str) -> list:
    """one value for all actors, or a sequence of P"""
    if hasattr(v, "tolist"):
        v = v.tolist()
    if not isinstance(v, (tuple, list)):
        return [v] * P
    if len(v) != P:
        raise ValueError(f"{name}: {len(v)} values for {P} actors")
    return list(v)


class _PopRollout:
    """swarm_pop_rollout launches of one configuration and P actors: the descriptor table in
    device memory and the [P, ...] result buffers the descriptors point into."""

    def __init__(self, lib, device, cfg: SwarmConfig, P: int):
        self.lib, self.device, self.cfg, self.P = lib, device, _copy_of(cfg), P
        self.table = torch.zeros(P * ctypes.sizeof(SwarmPopActor), dtype=torch.uint8, device=device)
        self._written = None   # the table's bytes as last copied to the device
        self._results = {}     # (n_ticks, traj) -> result dict

    def results(self, n_ticks: int, traj: bool) -> dict:
        res = self._results.get((n_ticks, traj))
        if res is None:
            P, B, N = self.P, self.cfg.n_envs, self.cfg.n_agents
            shapes = dict(reward=(P, B, N), hits=(P, B), avg_dist=(P, B), obs=(P, B, N, 6))
            if traj:
                shapes.update(traj_pos=(P, n_ticks, B, N, 2), traj_dist=(P, n_ticks, B), traj_hits=(P, n_ticks, B))
            res = self._results[n_ticks, traj] = {k: torch.zeros(s, device=self.device) for k, s in shapes.items()}
        return res

    def prepare(self, n_ticks: int, seeds, params, states, tick0, eps, traj: bool) -> dict:
        """Bring the device table in line with the arguments (pointers as integers; tick0 and eps
        one value or P) and return the result dict the next launch fills.  The table is copied to
        the device only when its bytes changed: a launch with the arguments of the one before
        touches nothing but the kernel's own buffers, so it can be captured and replayed; a
        ``prepare`` with new arguments between two replays holds from the next replay on."""
        P = self.P
        tick0, eps = _per_actor(tick0, P, "tick0"), _per_actor(eps, P, "eps")
        res = self.results(n_ticks, traj)
        arr = (SwarmPopActor * P)()
        for m in range(P):
            out = SwarmActOut(0, 0, ptr(res["reward"][m]), ptr(res["obs"][m]), ptr(res["avg_dist"][m]),
                              ptr(res["hits"][m]), 0, *[ptr(res[k][m]) if traj else 0
                                                        for k in ("traj_pos", "traj_dist", "traj_hits")])
            arr[m] = SwarmPopActor(seeds[m], params[m], states[m], out, int(tick0[m]) & 0xFFFFFFFF, float(eps[m]))
        raw = _bytes_of(arr)
        if raw != self._written:
            self.table.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))   # on the current stream
            self._written = raw
        return res

    def launch(self, n_ticks: int):
        if n_ticks == 0:   # nothing is written: a lone rollout's fresh (zero) results
            for traj in (False, True):
                for v in self._results.get((0, traj), {}).values():
                    v.zero_()
        call(self.lib, "swarm_pop_rollout", self.cfg, ptr(self.table), self.P, n_ticks)


class ActorPopulation:
    """P policies rolled out together: ``engines`` are existing ``SwarmEngine``s (``learn=False``
    or learners) on one device that share one configuration apart from the seed; ``rollout`` runs
    ``SwarmEngine.rollout`` of every one of them in ONE swarm_pop_rollout launch.  Row m of every
    result, and engine m's ``state`` / ``scenario_state`` afterwards, are bit for bit what
    ``engines[m].rollout(...)`` gives (tests/test_gpu_pop_rollout.py)."""

    def __init__(self, engines: Sequence[SwarmEngine]):
        engines = list(engines)
        if not engines:
            raise ValueError("an actor population needs at least one engine")
        first = engines[0]

        def shared(e):
            c = _copy_of(e.cfg)
            c.seed = 0
            return _bytes_of(c), e.device
        for e in engines:
            if shared(e) != shared(first):
                raise ValueError("the engines of an actor population share one device and one configuration (all "
                                 "but the seed): agents, envs, scenario, graph, conv, net")
        if len({id(e) for e in engines}) != len(engines):
            raise ValueError("an engine can be an actor only once")
        self.engines = engines
        self.P, self.B, self.N = len(engines), first.B, first.N
        self.lib, self.device = first.lib, first.device
        self._roll = _PopRollout(self.lib, self.device, first.cfg, self.P)
        self._params = None

    def prepare(self, n_ticks: int, tick0=0, eps=0.0, traj: bool = False, params=None) -> dict:
        """``rollout`` without the launch: the descriptor table is brought in line with the
        arguments (copied to the device only if they differ from the last call's) and the result
        dict is returned.  Between two replays of a captured ``rollout`` it changes what the next
        replay runs with (``n_ticks`` and ``traj`` are the capture's own)."""
        P = self.P
        if params is None:
            rows = [e.params for e in self.engines]
        else:
            n_par = self.engines[0].params.numel()
            if len(params) != P or (hasattr(params, "dim") and params.dim() != 2):
                raise ValueError(f"params: a [P, {n_par}] tensor or a list of {P} tensors")
            rows = [params[m] for m in range(P)]
            for r in rows:
                if r.numel() != n_par or r.dtype != torch.float32 or r.device != self.device or not r.is_contiguous():
                    raise ValueError(f"params: {n_par} contiguous float32 values on {self.device} per actor")
        self._params = rows   # kept alive while the table names them
        return self._roll.prepare(n_ticks, [e.cfg.seed for e in self.engines], [ptr(r) for r in rows],
                                  [ptr(e.state) for e in self.engines], tick0, eps, traj)

    def rollout(self, n_ticks: int, tick0=0, eps=0.0, traj: bool = False, params=None) -> dict:
        """``SwarmEngine.rollout`` of every engine in one launch: the same dict with a leading [P]
        dimension.  ``tick0`` and ``eps``: one value or P; ``params``: None (each engine's live
        ``params``), a [P, n_par] tensor or a list of P tensors.  The tensors returned are the
        population's own buffers, one set per (n_ticks, traj): the next rollout of that shape
        overwrites them.  The device descriptor table is rewritten only when an argument changed,
        so a rollout called once eagerly can then be captured and replayed (``prepare``)."""
        res = self.prepare(n_ticks, tick0, eps, traj, params)
        self._roll.launch(n_ticks)
        return res
