"""Rank sharding and the one data-path collective of the training tick.

* Environments shard contiguously: rank r of W owns the global envs
  [r*B, (r+1)*B).  ``swarm_config.env_offset = r*B`` keys every Philox draw
  (reset centre, ε coin, random actions, replay sampling) by the GLOBAL env
  index, so env e evolves identically whatever the rank layout.
* Each rank keeps its own replay ring and samples S graphs from it.
* The only exchange is a SUM all-reduce of the flat gradient buffer
  (1,673 parameters + the loss sum) once per TD update; every rank then applies
  clip_grad_norm_ + Adam to grad / W (``swarm_adam_cfg.world_size``), so the
  replicas stay bit-identical.  The loss is a mean over nodes, hence with equal
  per-rank S this is the single-process update over the union batch
  (tests/test_dist_gloo.py checks it with the oracle on two gloo ranks).

One process per GPU; on ROCm the ``nccl`` backend of torch.distributed is RCCL
(xGMI between the GPUs of a node).  The 6.7 KB message is latency-bound: one
call per update, issued on the compute stream.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass(frozen=True)
class Shard:
    rank: int
    world_size: int
    envs_per_rank: int

    @property
    def env_offset(self) -> int:
        return self.rank * self.envs_per_rank

    @property
    def global_envs(self) -> int:
        return self.world_size * self.envs_per_rank

    def env_range(self) -> range:
        return range(self.env_offset, self.env_offset + self.envs_per_rank)


def shard_from_env(envs_per_rank: int) -> Shard:
    """Shard of this process from torchrun's RANK / WORLD_SIZE (1 rank if unset)."""
    return Shard(int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), envs_per_rank)


def init_process_group(backend: str, local_rank: Optional[int] = None):
    """torch.distributed.init_process_group for a torchrun launch (MASTER_ADDR 127.0.0.1)."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    kw = {}
    if backend == "nccl" and local_rank is not None:
        kw["device_id"] = torch.device("cuda", local_rank)
    dist.init_process_group(backend, **kw)
    return dist.group.WORLD


def allreduce_grad_(grad: torch.Tensor, world_size: int, group=None, peer: "PeerExchange" = None) -> torch.Tensor:
    """In-place SUM of the flat gradient over ranks (no-op for one rank without a group).
    The division by W happens inside the optimizer step (swarm_adam_cfg.world_size).
    With a PeerExchange the sum runs as swarm_peer_allreduce (xGMI stores), else over RCCL."""
    if peer is not None:
        peer.allreduce_(grad)
    elif world_size > 1 or group is not None:
        import torch.distributed as dist
        dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=group)
    return grad


class PeerExchange:
    """One rank's end of the peer all-reduce (include/swarm_hip.h "Peer all-reduce over xGMI").

    The rank allocates one uncached exchange buffer (``swarm_peer_alloc``), exports its HIP IPC
    handle, gathers every rank's handle over the process group (the group carries only this
    setup and the bench's barriers; the data path never touches it) and maps the others'
    buffers.  ``SwarmEngine.train_tick`` then runs ``swarm_reduce_advance_peer``: the slab
    reduce, the exchange and the rank-ordered sum in ONE launch, graph-capturable, with no RCCL
    call.  Every rank must issue the same sequence of peer launches (SPMD), as with a collective.

    ``local(W)`` builds W ends in one process over W local buffers: the single-GPU emulation
    the tests use (W engines on W streams)."""

    def __init__(self, lib, world_size: int, rank: int, own: int, recv: list, device, owned: list,
                 mapped: list, timeout_us: int = 0):
        from ._lib import PEER_MAX, PEER_SEQ_WORDS, SwarmPeer, c_void_p
        self.lib, self.world_size, self.rank, self.device = lib, world_size, rank, torch.device(device)
        self.own, self._owned, self._mapped = own, owned, mapped
        self.seq = torch.zeros(PEER_SEQ_WORDS, dtype=torch.int32, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        arr = (c_void_p * PEER_MAX)()
        for q, p in enumerate(recv):
            arr[q] = p
        self.struct = SwarmPeer(world_size, rank, arr, self.seq.data_ptr(), self.err.data_ptr(), int(timeout_us), 0)
        self.error = None   # connect(): the first failed IPC mapping, if any
        self._stream = None  # the one stream this rank's peer launches are ordered on (check_stream)

    # ------------------------------------------------------------------ construction
    @staticmethod
    def _alloc(lib) -> int:
        from ._lib import c_void_p, call
        import ctypes
        p = c_void_p()
        call(lib, "swarm_peer_alloc", ctypes.byref(p))
        return int(p.value)

    @classmethod
    def connect(cls, group=None, device=None, timeout_us: int = 0) -> "PeerExchange":
        """Collective over ``group`` (every rank calls it): allocate, exchange IPC handles, map.

        Never raises on one rank alone: a failure to allocate, to export the handle or to map a
        peer's buffer is recorded in ``.error`` and the rank still enters every collective of the
        setup (the handle gather and the barrier), so the ranks' collectives stay matched and
        ``selftest()`` then fails on it without launching.  A world larger than
        SWARM_PEER_MAX raises ValueError on every rank alike, before any collective."""
        import ctypes
        import torch.distributed as dist
        from . import _lib
        lib = _lib.load()
        W, r = dist.get_world_size(group), dist.get_rank(group)
        if W > _lib.PEER_MAX:
            raise ValueError(f"peer all-reduce supports up to {_lib.PEER_MAX} ranks (one node), got {W}")
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        err, own, mine = None, None, None
        try:
            own = cls._alloc(lib)
            h = (ctypes.c_char * _lib.PEER_HANDLE_BYTES)()
            _lib.call(lib, "swarm_peer_ipc_handle", ctypes.c_void_p(own), h)
            mine = bytes(h)
        except RuntimeError as e:   # keep going: this rank still joins the gather and the barrier
            err = e
        handles = [None] * W
        dist.all_gather_object(handles, mine, group=group)
        recv, mapped = [], []
        for q, hq in enumerate(handles):
            if q == r:
                recv.append(own)
                continue
            if hq is None:   # that rank has no buffer: its own error says why
                err = err or RuntimeError(f"peer all-reduce: rank {q} could not set up its exchange buffer")
                recv.append(None)
                continue
            p = ctypes.c_void_p()
            buf = (ctypes.c_char * _lib.PEER_HANDLE_BYTES).from_buffer_copy(hq)
            try:
                _lib.call(lib, "swarm_peer_ipc_open", buf, ctypes.byref(p))
            except RuntimeError as e:   # keep going: every rank must still reach the barrier below
                err = err or RuntimeError(f"{e} (the buffer of rank {q})")
                recv.append(None)
                continue
            recv.append(int(p.value))
            mapped.append(int(p.value))
        dist.barrier(group)
        end = cls(lib, W, r, own or 0, [x or 0 for x in recv], dev, [own] if own else [], mapped, timeout_us)
        # a failed mapping does not raise here: this rank's buffer must stay allocated while the
        # others (who mapped it) still run their self-test; selftest() then reports the failure
        # on this rank without launching, and the others' waits expire on it (bench.py falls
        # back to RCCL on every rank together)
        end.error = err
        return end

    @classmethod
    def local(cls, world_size: int, device=None, timeout_us: int = 0) -> list:
        """W ends in one process (single-GPU emulation of W ranks)."""
        from . import _lib
        lib = _lib.load()
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        bufs = [cls._alloc(lib) for _ in range(world_size)]
        ends = [cls(lib, world_size, r, bufs[r], bufs, dev, [], [], timeout_us) for r in range(world_size)]
        ends[0]._owned = bufs   # the first end frees them all
        return ends

    # ------------------------------------------------------------------ use
    def check_stream(self):
        """The exchange's double-buffer argument (swarm_peer.h: parity s & 1 is safe because a
        rank's launch s + 2 follows its launch s in STREAM ORDER) holds only if every peer
        launch of this rank is ordered on one stream.  The first eager launch binds that stream;
        an eager launch from another stream raises.  Launches recorded into a hipGraph are not
        checked here: replay the graph on the bound stream (SwarmEngine and bench.py do)."""
        if torch.cuda.is_current_stream_capturing():
            return
        cur = torch.cuda.current_stream(self.device)
        if self._stream is None:
            self._stream = cur
        elif cur != self._stream:
            raise RuntimeError("peer all-reduce: every peer launch of a rank must be on one stream (the first "
                               f"eager launch used {self._stream}, this one {cur}); unordered launches could reuse "
                               "a parity slot of the exchange buffer before the other ranks read it")

    def allreduce_(self, x: torch.Tensor) -> torch.Tensor:
        """In-place rank-ordered SUM of a flat fp32 device tensor (<= 1,674 elements), launched on
        the current stream, which must be this rank's one peer stream (``check_stream``)."""
        from ._lib import call
        assert x.is_contiguous() and x.dtype == torch.float32 and x.device == self.device
        self.check_stream()
        call(self.lib, "swarm_peer_allreduce", self.struct, x.data_ptr(), x.numel())
        return x

    def errors(self) -> int:
        """Exchange waits that expired (0 in a correct run); one 4-byte device read."""
        return int(self.err.item())

    def check(self):
        n = self.errors()
        if n:
            raise RuntimeError(f"peer all-reduce: {n} exchange wait(s) expired (a rank stopped issuing the same "
                               "sequence of peer launches, or its stores never arrived); the gradients are wrong")

    def selftest(self) -> bool:
        """Every rank contributes (rank + 1) * (1 + column): the rank-ordered sums are exact
        small integers.  Returns False on a wrong sum, an expired wait or a failed IPC mapping at
        connect() (caller falls back)."""
        from ._lib import N_PARAMS
        if self.error is not None:
            return False
        n = N_PARAMS + 1
        st = self._stream if self._stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):   # on this rank's peer stream (check_stream)
            col = torch.arange(n, dtype=torch.float32, device=self.device)
            x = (self.rank + 1) * (1 + col)
            self.allreduce_(x)
            want = (self.world_size * (self.world_size + 1) / 2) * (1 + col)
            ok = bool(torch.equal(x, want)) and self.errors() == 0
        return ok

    def fused_selftest(self, make_engine, group=None, ticks: int = 4) -> dict:
        """The exchange the timed ticks will run, executed before them on THIS library (VERDICT r5
        "next" #2): ``make_engine(peer)`` builds a throwaway engine of the run's configuration
        (same envs, agents and TD batch, hence the same tick kernel, slab count and reduce
        geometry) on this exchange; ``ticks`` training ticks then go through
        ``swarm_reduce_advance_peer`` (grad_reduce_kernel<1>: slab sum, peer stores, rank-ordered
        sum).  After each, this rank's own column sums of the same slabs (``swarm_grad_reduce``:
        the same geometry, no exchange) are gathered over ``group`` and the gradient every rank
        holds must equal their rank-ordered fp32 sum bit for bit; the expired-wait word, the
        hand-off word and ctrl.peer_hold must stay 0.  Collective: every rank calls it.  Returns
        {"ok": bool, ...details}; the caller MIN-reduces "ok" over the ranks and falls back."""
        import torch.distributed as dist
        from . import _lib
        from ._lib import CTRL, N_PARAMS, call, ptr
        if self.error is not None:
            return {"ok": False, "why": str(self.error)}
        eng = make_engine(self)
        if eng.peer is not self:
            raise ValueError("fused_selftest: make_engine must build its engine on this exchange")
        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        local = torch.zeros_like(eng.grad)
        res, nonzero = [], 0
        st = self._stream if self._stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):   # this rank's one peer stream (check_stream)
            eng.reset(0)
            for t in range(ticks):
                eng.train_tick()
                call(self.lib, "swarm_grad_reduce", eng.cfg, eng.hp, ptr(eng.slabs), ptr(local))
                torch.cuda.synchronize(self.device)
                mine = local[:N_PARAMS + 1].clone()
                allv = [torch.zeros_like(mine, device=dev) for _ in range(self.world_size)]
                dist.all_gather(allv, mine.to(dev), group=group)
                want = allv[0].clone()
                for q in range(1, self.world_size):
                    want = want + allv[q]   # rank order, fp32
                got = eng.grad[:N_PARAMS + 1].to(dev)
                res.append(bool(torch.equal(got, want)))
                nonzero += int(bool(mine.abs().sum() > 0))
            eng.flush()
            torch.cuda.synchronize(self.device)
        out = {"ok": all(res) and nonzero > 0 and self.errors() == 0 and eng.handoff_errors() == 0
               and int(eng.ctrl[CTRL["peer_hold"]].item()) == 0,
               "ticks": ticks, "bitwise": sum(res), "trained_ticks": nonzero, "expired_waits": self.errors(),
               "handoff_overruns": eng.handoff_errors(), "peer_hold": int(eng.ctrl[CTRL["peer_hold"]].item()),
               "reduce_geometry": _lib.load().swarm_build_info().decode()}
        del eng
        return out

    def close(self):
        from ._lib import call
        import ctypes
        for p in self._mapped:
            call(self.lib, "swarm_peer_ipc_close", ctypes.c_void_p(p))
        for p in self._owned:
            call(self.lib, "swarm_peer_free", ctypes.c_void_p(p))
        self._mapped, self._owned = [], []
