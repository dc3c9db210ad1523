"""Headline benchmark: env-steps/sec (agents x envs) of the fused swarm-RL training
tick, GoTo, 8 agents x 1024 envs per GPU (BASELINE.json configs[1]; weak scaling
to configs[3] = 8192 envs over 8 GPUs).

One step = one training EPISODE of the reference's hot loop (train_gcn_dqn.py:153-178:
reset_world_at, then max_steps = 100 ticks) for every env of every rank.  One tick:
GAT Q forward on the complete graph -> ε-greedy (ε = 0.05) -> VMAS env.step -> replay
push -> TD update on S = 1024 sampled graphs per rank (target fwd, online fwd, backward)
-> [RCCL all-reduce of the 1,673-float gradient] -> clip_grad_norm_ + Adam (+ target
sync every 200 ticks).  A 100-tick step keeps the timed region well above launch and
sync noise at the driver's K (20 steps = 2,000 ticks); `tick_us` reports the spread of
the per-episode times (HIP events between steps).  Inputs: synthetic reset states
(Philox), weights data/models/experiment_GoTo-seed_0.pth (committed fixture), replay
pre-filled with 100 acting ticks.  Each episode's 100 ticks replay one captured hipGraph.

A plain run sets up, warms up, times the K steps and prints the result line.  --full adds,
after the timed region, everything else the line can report: per-kernel durations and the
roofline, the acting-only rollouts, the CPU baselines (and at N > 1 the second timed region
over RCCL).  --dump-outputs DIR writes what the last timed step left a caller (dump_outputs).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
       N > 1 under a launcher (torch.distributed.run --nproc-per-node N ... bench.py --gpus N): one
       rank per process as the launcher started them.  N > 1 without one (WORLD_SIZE unset): this
       process starts the N ranks itself (a torch.distributed.run child, before any GPU call), relays
       their output and exits non-zero if a rank fails or the JSON line's n_gpus is not N.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import platform
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_TFLOPS = 157.3     # MI355X FP32 MFMA (= vector) dense peak, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0        # HBM3E spec
PEAK_CLOCK_GHZ = 2.4         # the clock the FP32 peak is quoted at (1024 SIMDs x 64 FLOP/cycle)


def gat_fwd_flops(N: int, avg_in_degree: float) -> float:
    """Algorithmic FLOPs of GCN.forward per node: lin 7->32 (448), scores (128),
    softmax (5/edge), aggregate (64/edge), bias+tanh (64), lin1 (2048+32), relu (32), lin2 (576+9)."""
    return 448 + 128 + 69 * avg_in_degree + 64 + 2080 + 32 + 585


def td_bwd_flops(N: int, d: float) -> float:
    """Algorithmic FLOPs of the TD backward per sampled node."""
    return (32 + 32 + 2048 + 96        # dR (one-hot row), relu mask, W1^T dZ, tanh'
            + 64 * d + 8 * d + 64 * d  # g_uv, softmax/leaky backward, messages to h
            + 128 + 128                # attention-vector terms into dh, datt
            + 2048 + 64 + 448          # dW1, dW2 (one-hot), dW
            + 32 * 3 + 9)              # dbias, db1, db2


def gcn_fwd_flops(N: int, d: float) -> float:
    """GCNConv variant (a13) per node: lin 7->32 (448), normalised aggregate (64/edge + 3/edge
    coefficients), bias+tanh (64), lin1, relu, lin2 as for the GAT."""
    return 448 + 67 * d + 64 + 2080 + 32 + 585


def gat3_fwd_flops(N: int, d: float) -> float:
    """The Flocking checkpoints' three-layer GAT (hidden 8) per node: lins 7->8 (112) and 8->8
    (2 x 128), scores (3 x 32), softmax + aggregate per edge (3 x (5 + 16)), bias + activation
    (3 x 16), lin1 (128 + 8), relu (8), lin2 (144 + 9)."""
    return 112 + 256 + 96 + 63 * d + 48 + 136 + 8 + 153


def gcn_bwd_flops(N: int, d: float) -> float:
    return 32 + 32 + 2048 + 96 + 64 * d + 2048 + 64 + 448 + 32 * 2 + 9


def complete_in_degree(N: int) -> float:
    return ((N - 1) * N + 1) / N


def mean_in_degree(args, eng) -> float:
    """Average in-degree of the bench graph: analytic for complete / kNN, measured on the
    reset state for the radius graph (its degree depends on the formation)."""
    N = args.agents
    if args.graph == "complete":
        return complete_in_degree(N)
    if args.graph == "knn":
        return (2 * N * args.knn_k + 1) / N
    import swarm_amd
    eng.reset(0)
    obs = torch.cat([eng.state, torch.tensor([-0.8, 0.8], device=eng.state.device).expand(*eng.state.shape[:2], 2)], -1)
    d = swarm_amd.create_radius_graph_from_observations(obs, N, args.radius)
    from swarm_amd.graph import build_mult
    return float(build_mult(d).float().sum().item()) / (args.envs * N)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (training: episodes of --ticks ticks)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=100, help="ticks per step = per episode (max_steps, "
                    "train_gcn_dqn.py:149)")
    ap.add_argument("--envs", type=int, default=1024, help="envs per GPU")
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--scenario", default="GoTo")
    ap.add_argument("--conv", default="gat", choices=("gat", "gcn"))
    ap.add_argument("--graph", default="complete", choices=("complete", "knn", "radius"))
    ap.add_argument("--knn-k", type=int, default=10)
    ap.add_argument("--radius", type=float, default=0.3, help="neighbour radius of --graph radius")
    ap.add_argument("--mode", default="train", choices=("train", "act"),
                    help="train: fused training tick (headline); act: acting-only rollout with frozen "
                         "weights, eps 0 (Simulator-shaped, replicas only)")
    ap.add_argument("--tick", default="fused", choices=("fused", "3"),
                    help="fused: acting + TD blocks in one launch (swarm_train_tick) where supported; "
                         "3: act / TD / reduce launches")
    ap.add_argument("--net", default="gcn", choices=("gcn", "gat3"),
                    help="gat3: the Flocking checkpoints' three-layer GAT (acting only, --mode act)")
    ap.add_argument("--batch", type=int, default=None, help="sampled graphs per update per GPU (default = envs)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also measure the per-kernel durations and roofline, the "
                         "acting-only rollouts and the CPU baselines (N > 1: the RCCL timed region as well)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step left (state, per-tick outputs, learner) as "
                         "DIR/<name>.npy, float32")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; "
                    "gloo only to rehearse several ranks on one GPU)")
    ap.add_argument("--force-dist", action="store_true",
                    help="rehearsal: create the process group and run the gradient all-reduce even at 1 rank")
    ap.add_argument("--no-compare-rccl", dest="compare_rccl", action="store_false",
                    help="N > 1 with the peer exchange: skip the second timed region over RCCL")
    ap.add_argument("--c1-seconds", type=float, default=5.0, help="CPU sample of BASELINE configs[0] (C1)")
    ap.add_argument("--allreduce", default="auto", choices=("auto", "peer", "rccl"),
                    help="gradient all-reduce for N > 1: peer = xGMI stores fused into the slab reduce "
                         "(swarm_reduce_advance_peer); rccl = torch.distributed all_reduce after it; auto = peer "
                         "if its setup self-test passes on every rank, else rccl")
    return ap.parse_args()


def launch_decision(gpus: int, env) -> str:
    """How this process runs --gpus N: "run" (one rank: N == 1, or a launcher set WORLD_SIZE == N)
    or "spawn" (N > 1 and no launcher: start the N ranks first).  A launcher's WORLD_SIZE that
    differs from N is an error (SystemExit): the line would be quoted for the wrong GPU count."""
    if gpus < 1:
        raise SystemExit(f"--gpus {gpus}: need at least one GPU")
    ws = env.get("WORLD_SIZE")
    if ws is None:
        return "spawn" if gpus > 1 else "run"
    if int(ws) != gpus:
        raise SystemExit(f"--gpus {gpus} but WORLD_SIZE={ws}")
    return "run"


def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_launch_cmd(argv, n: int, port: int, script: str = None):
    """torch.distributed.run command that starts n ranks of this script with the same arguments
    (one node, rendezvous on 127.0.0.1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr=127.0.0.1", f"--master-port={port}", script or os.path.abspath(__file__), *argv]


def spawn_ranks(argv, n: int, script: str = None) -> int:
    """Start n ranks as a child process (never an exec: this process has not touched the GPU and
    stays the parent), relay their stdout line by line, and return non-zero if the launcher fails
    or rank 0's JSON line does not report n GPUs."""
    import signal
    cmd = rank_launch_cmd(argv, n, free_port(), script)
    print("[bench] starting %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    # own session: on any exit of the relay other than its normal end (an exception, ^C, SIGTERM or
    # SIGHUP, which the handlers below turn into SystemExit) the whole launcher process group is
    # terminated, ranks included; the ranks are outside the caller's process group, so without
    # the handlers a SIGTERM to the relay would orphan them
    def _exit_on(signum, _frame):
        raise SystemExit(128 + signum)
    old = {sig: signal.signal(sig, _exit_on) for sig in (signal.SIGTERM, signal.SIGHUP)}
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, bufsize=1, start_new_session=True)
    line = None
    done = False
    try:
        for raw in proc.stdout:
            sys.stdout.write(raw)
            sys.stdout.flush()
            if raw.lstrip().startswith("{"):
                try:
                    d = json.loads(raw)
                except ValueError:
                    continue
                if "n_gpus" in d:
                    line = d
        rc = proc.wait()
        done = True
    finally:
        if not done:
            stop_group(proc)
        for sig, h in old.items():
            signal.signal(sig, h)
    if rc != 0:
        print(f"[bench] rank launcher exited with {rc}", file=sys.stderr)
        return rc
    if line is None or line.get("n_gpus") != n:
        print(f"[bench] expected a JSON line with n_gpus {n}, got {None if line is None else line.get('n_gpus')}",
              file=sys.stderr)
        return 3
    return 0


def stop_group(proc, grace: float = 10.0) -> None:
    """SIGTERM the launcher's process group (it leads its own session), SIGKILL after `grace` s."""
    import signal
    for sig in (signal.SIGTERM, signal.SIGKILL):
        try:
            os.killpg(proc.pid, sig)
        except (ProcessLookupError, PermissionError):
            return
        try:
            proc.wait(timeout=grace)
            return
        except subprocess.TimeoutExpired:
            continue


def main():
    args = parse()
    if launch_decision(args.gpus, os.environ) == "spawn":
        sys.exit(spawn_ranks(sys.argv[1:], args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:   # launch_decision guarantees it; kept as the invariant the line relies on
        raise SystemExit(f"--gpus {args.gpus} but world size {world}")
    torch.cuda.set_device(local_rank % max(1, torch.cuda.device_count()))   # several gloo ranks may share a GPU
    distributed = world > 1 or args.force_dist
    import swarm_amd
    from swarm_amd import dist as swdist
    pg = swdist.init_process_group(args.backend, local_rank) if distributed else None
    from swarm_amd import build as swbuild
    # an explicit SWARM_LIB_PATH (A/B runs of a prebuilt library) is never rebuilt here
    if rank == 0 and not os.environ.get("SWARM_LIB_PATH") and not swbuild.up_to_date():
        swbuild.build()
    if distributed:
        torch.distributed.barrier()

    build = lib_identity()
    B, N = args.envs, args.agents
    shard = swdist.Shard(rank, world, B)
    S = args.batch or B
    scen = args.scenario
    if args.net == "gat3":
        if args.mode != "act":
            raise SystemExit("--net gat3 is forward only: use --mode act")
        w0 = torch.tensor(np.load(os.path.join(ROOT, "tests", "golden", "flocking_weights.npz"))["weights_flocking"][0])
    else:   # Flocking trains the one-layer network: start it from GoTo's checkpoint
        wkey = "weights_obstacle_avoidance" if scen == "ObstacleAvoidance" else "weights_go_to"
        w0 = torch.tensor(np.load(os.path.join(ROOT, "tests", "golden", "weights.npz"))[wkey][0])
    peer, allreduce, fused_check = None, None, None
    if distributed and args.mode == "train":
        allreduce = "rccl" if args.backend == "nccl" else args.backend
        if args.allreduce != "rccl":
            why = None
            try:
                peer = swdist.PeerExchange.connect(pg)
                ok = peer.selftest()
                if not ok and peer.error is not None:   # an IPC mapping failed on this rank
                    why = str(peer.error)
            except (RuntimeError, ValueError) as e:   # IPC unavailable; W > SWARM_PEER_MAX (every rank alike)
                why, ok = str(e), False
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32,
                                device="cuda" if args.backend == "nccl" else "cpu")
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            if int(flag.item()) == 1:
                # VERDICT r5 "next" #2: before any timed tick, the exchange the line will time runs on
                # THIS library: fused training ticks of the run's own configuration through
                # swarm_reduce_advance_peer (the shipped reduce geometry), every rank's gradient checked
                # bitwise against the rank-ordered sum of the ranks' own column sums, error words 0
                try:
                    fused_check = peer.fused_selftest(lambda p: swarm_amd.SwarmEngine(
                        scen, N, B, seed=0, params=w0, batch=S, eps=0.05, env_offset=shard.env_offset,
                        world_size=world, process_group=pg, update_target_every=2, replay_capacity=3 * B,
                        conv=args.conv, graph=args.graph, knn_k=args.knn_k, radius=args.radius, peer=p), pg)
                except RuntimeError as e:
                    fused_check = {"ok": False, "why": str(e)}
                flag.fill_(1 if fused_check["ok"] else 0)
                torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
                fused_check["all_ranks_ok"] = int(flag.item()) == 1
                if not fused_check["ok"]:
                    why = f"fused exchange check: {fused_check}"
            if int(flag.item()) == 1:
                allreduce = "xGMI peer stores fused into the slab reduce (swarm_reduce_advance_peer)"
            else:
                if args.allreduce == "peer":
                    raise SystemExit(f"rank {rank}: peer all-reduce self-test failed ({why or 'wrong sums'})")
                print(f"[bench] rank {rank}: peer all-reduce self-test failed ({why or 'wrong sums on a peer rank'}); "
                      f"falling back to {allreduce}", file=sys.stderr)
                peer = None

    eng = swarm_amd.SwarmEngine(scen, N, B, seed=0, params=w0, batch=S, eps=0.05, env_offset=shard.env_offset,
                                world_size=world, process_group=pg, update_target_every=200,
                                replay_capacity=1_000_000 if args.net == "gcn" else 1, conv=args.conv,
                                graph=args.graph, knn_k=args.knn_k, radius=args.radius, net=args.net,
                                learn=args.net == "gcn", peer=peer)
    max_steps = args.ticks
    if args.mode == "act":
        return bench_act(args, eng, world, rank, distributed, max_steps)
    # ---- prefill: 100 acting ticks (no learning)
    eng.reset()
    for _ in range(100):
        eng.act(push=True, full_out=False)
        eng.advance()
    eng.reset()

    fused = eng.fused and args.tick == "fused"

    def tick():
        if fused:
            eng.train_tick(full_out=False)
        else:
            eng.train_tick3(full_out=False)

    stream = torch.cuda.current_stream()

    def timed_region():
        """capture one episode's ticks (hipGraph), W warmup steps, then K timed steps between a
        barrier + synchronize on both sides; returns (max-over-ranks seconds, tick spread, graph?)"""
        graph = None
        if not args.no_graph and (not distributed or args.backend == "nccl" or eng.peer is not None):
            tick()                              # eager warm tick (and first RCCL all-reduce) before capture
            try:
                graph = eng.capture(max_steps, tick)   # one episode's ticks
            except RuntimeError as e:           # e.g. a collective that refuses stream capture
                print(f"[bench] rank {rank}: hipGraph capture failed ({e}); eager ticks", file=sys.stderr)
                graph = None
            if distributed:                     # every rank runs the same launch mode
                ok = torch.tensor([1 if graph is not None else 0], dtype=torch.int32,
                                  device="cuda" if args.backend == "nccl" else "cpu")
                torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN)
                if int(ok.item()) == 0:
                    graph = None

        def episode():   # one step: reset_world_at, then max_steps ticks
            eng.reset()
            if graph is not None:
                graph.replay()
            else:
                for _ in range(max_steps):
                    tick()

        for _ in range(args.warmup):
            episode()
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        t0 = time.perf_counter()
        evs[0].record(stream)
        for i in range(args.steps):
            episode()
            evs[i + 1].record(stream)
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        ep_us = [evs[i].elapsed_time(evs[i + 1]) * 1e3 / max_steps for i in range(args.steps)]
        spread = ({"median": round(float(np.median(ep_us)), 3), "min": round(min(ep_us), 3),
                   "max": round(max(ep_us), 3), "per": "episode of %d ticks, HIP events" % max_steps}
                  if ep_us else None)
        if distributed:
            t = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, spread, graph

    elapsed, tick_spread, graph = timed_region()
    if args.dump_outputs:   # before anything below touches the engine again
        dump_outputs(args.dump_outputs, train_outputs(eng), rank, world)
    # --full, N > 1 with the peer exchange: the same workload again with the RCCL all-reduce after the
    # slab reduce (north_star's "single RCCL all-reduce over xGMI"), so one run reports both paths
    both = None
    if args.full and distributed and peer is not None and args.backend == "nccl" and args.compare_rccl:
        peer.check()
        el_peer = elapsed
        eng.peer = None
        el_rccl, spread_rccl, g_rccl = timed_region()
        eng.peer = peer
        both = {"peer": {"value": round(B * N * world * args.steps * max_steps / el_peer, 1),
                         "us_per_tick": round(el_peer / (args.steps * max_steps) * 1e6, 3)},
                "rccl": {"value": round(B * N * world * args.steps * max_steps / el_rccl, 1),
                         "us_per_tick": round(el_rccl / (args.steps * max_steps) * 1e6, 3),
                         "tick_us": spread_rccl, "hipgraph": g_rccl is not None},
                "headline": "peer"}
    ctrl = eng.read_ctrl()
    assert ctrl["trained"] == 1 and math.isfinite(ctrl["loss"]), ctrl
    rank_errors = None
    if distributed:   # every rank's fused-tick hand-off overruns and expired exchange waits (0 in a correct run)
        e = torch.tensor([eng.handoff_errors(), peer.errors() if peer is not None else 0,
                          int(eng.ctrl[23].item())], dtype=torch.int64,
                         device="cuda" if args.backend == "nccl" else "cpu")
        allv = [torch.zeros_like(e) for _ in range(world)]
        torch.distributed.all_gather(allv, e)
        rank_errors = [{"rank": q, "handoff_overruns": int(v[0]), "peer_wait_expired": int(v[1]),
                        "peer_hold": int(v[2])} for q, v in enumerate(allv)]
    if peer is not None:
        peer.check()   # an expired exchange wait would have summed a wrong gradient: fail loudly
    replicas = None
    if distributed:
        # data-parallel invariant: after the same all-reduced updates every replica's weights,
        # moments and target are bitwise identical (min == max over ranks, element by element)
        eng.flush()
        st = torch.cat([eng.params, eng.adam_m, eng.adam_v, eng.target])
        lo, hi = st.clone(), st.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        replicas = bool(torch.equal(lo, hi))
        if not replicas:
            raise SystemExit(f"rank {rank}: replicas diverged after {args.steps} ticks")

    value = B * N * world * args.steps * max_steps / elapsed
    ms = elapsed / args.steps * 1e3          # per step (episode)
    tick_ms = ms / max_steps

    # ---- per-kernel durations, each as the period of a captured chain of real launches timed with
    #      HIP events on the stream the graph launches on (a period holds the kernel and one launch
    #      boundary).  Fused tick: tick_kernel = period of (tick launch, swarm_ctrl_advance) pairs
    #      minus the period of the advance alone (every tick launch advances the tick counter and the
    #      replay slot, so its hand-off waits are real); reduce_advance = period of the slab reduce
    #      alone; tick_period = period of whole ticks (tick launch + reduce), the tick without the
    #      timed region's per-episode reset.  3-launch tick: each kernel's chain (TD and the slab
    #      reduce are pure functions of their inputs).
    kt = {}
    if args.full and not args.no_kernel_timing:
        stream = torch.cuda.current_stream()

        def chain_us(fn, kchain=50):
            fn()
            g = eng.capture(kchain, fn)
            per = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                g.replay()
                e1.record(stream)
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / kchain)
            return float(np.median(per))   # microseconds per launch

        if fused:
            eng.reset()
            t_pair = chain_us(lambda: (eng.launch_tick(), eng.advance()), 40)
            t_adv = chain_us(eng.advance, 40)
            kt["tick_kernel"] = t_pair - t_adv
            kt["ctrl_advance_kernel (an empty launch's period)"] = t_adv
            if eng.peer is None and world == 1:
                kt["reduce_advance (period)"] = chain_us(eng.launch_reduce_advance, 40)
                kt["tick_period (tick + reduce)"] = chain_us(lambda: (eng.launch_tick(), eng.launch_reduce_advance()), 40)
            eng.flush()
            eng.reset()
            assert eng.handoff_errors() == 0, "fused tick: a hand-off wait hit its bound"
        else:
            for name, fn in (("td_kernel", eng.launch_td), ("act_kernel", eng.launch_train_act),
                             ("grad_reduce_kernel", eng.launch_grad_reduce)):
                kt[name] = chain_us(fn)

    d = mean_in_degree(args, eng) if kt else 0.0   # the roofline's FLOP counts only
    if args.conv == "gat":
        td_flops_launch = S * N * (2 * gat_fwd_flops(N, d) + td_bwd_flops(N, d))
    else:
        td_flops_launch = S * N * (2 * gcn_fwd_flops(N, d) + gcn_bwd_flops(N, d))
    # acting half per agent-step: forward + ~300 FLOP of physics; 69 B (state r/w 32 + push 37)
    act_flops_launch = B * N * ((gat_fwd_flops(N, d) if args.conv == "gat" else gcn_fwd_flops(N, d)) + 300)
    roof = None
    if kt:
        headline = (scen, N, B, S, args.conv, args.graph) == ("GoTo", 8, 1024, 1024, "gat", "complete")
        if fused:   # the dominant kernel is the whole fused tick kernel (acting + TD blocks)
            t_k = kt["tick_kernel"] * 1e-6
            flops, nbytes = act_flops_launch + td_flops_launch, B * N * 69 + S * N * 37
            kname, pmcf = "tick_kernel (swarm_train_tick: acting + TD blocks)", "tick"
        else:
            t_k = kt["td_kernel"] * 1e-6
            flops, nbytes = td_flops_launch, S * N * 37
            kname, pmcf = "td_kernel (swarm_td_grad)", "td"
        ach = flops / t_k / 1e12
        traffic, mfma_util, pmc_src = None, None, None
        if headline:   # counters only from a profile of THIS library build (tools/pmc_summary.py)
            pmc_src = find_pmc(pmcf, build)
            if pmc_src.get("file"):
                dd = pmc_src.pop("data")
                traffic = dd.get("hbm_bytes_per_launch")
                kk = dd.get("kernels", {}).get(dd.get("kernel", ""), {}).get("counters", {})
                busy = kk.get("SQ_VALU_MFMA_BUSY_CYCLES")
                if busy is not None:   # MFMA pipe cycles / (1024 SIMDs x this launch's time at the 2.4 GHz peak clock)
                    mfma_util = busy / (1024 * PEAK_CLOCK_GHZ * 1e9 * t_k)
        else:
            pmc_src = {"file": None, "reason": "counters are collected for the headline configuration only"}
        roof = {"bound": "valu" if args.net == "gat3" else "mfma", "achieved": round(ach, 4),
                "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
                "frac": ach / PEAK_FP32_TFLOPS, "traffic": traffic, "kernel": kname,
                "algorithmic_flops_per_launch": flops,
                "algorithmic_bytes_per_launch": nbytes,
                "hbm_frac": nbytes / t_k / 1e9 / PEAK_HBM_GBS,
                "hbm_gbs": round(traffic / t_k / 1e9, 1) if traffic else None,
                "mfma_util": mfma_util, "pmc": pmc_src,
                "kernel_us": {k: round(v, 2) for k, v in kt.items()}}

    # SURVEY §8(d)'s second number: acting-only (S = 0, frozen weights, eps 0, like
    # Simulator.run_simulation), one swarm_rollout launch per max_steps-tick episode, after the
    # timed region, one GPU only.  The headline acting line runs the reference's EVALUATION graph,
    # kNN with k = min(10, N) (simulator.py:19 uses k = 10, which needs N >= 10; at 8 agents the
    # recorded evaluations ran k = 5, data/test_stats); the training graph (this engine's) is
    # reported beside it, labelled
    acting = None
    if args.full and world == 1:
        import swarm_amd
        k_eval = min(10, N) if N >= 10 else min(5, N)
        e_knn = swarm_amd.SwarmEngine(scen, N, B, seed=0, params=w0, graph="knn", knn_k=k_eval, conv=args.conv,
                                      learn=False, eps=0.0)
        acting = acting_leg(argparse.Namespace(**{**vars(args), "graph": "knn", "knn_k": k_eval}), e_knn, max_steps)
        del e_knn
        acting["training_graph"] = acting_leg(args, eng, max_steps)
        # the basis of this key changed in round 5; say so in the line itself
        acting["headline_graph"] = (f"kNN-{k_eval}: the reference's evaluation graph (simulator.py:15-24), the "
                                    "basis of acting_only.value since round 5; rounds 1-4 quoted the training "
                                    "graph's rollout, which is acting_only.training_graph")

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline_leg(args, w0, scen, B, N, S, eng)

    if rank == 0:
        line = {"metric": "env-steps/sec (agents×envs), GoTo 8 agents×1024 envs @1/2/4/8 GPU",
                "value": round(value, 1), "unit": "agent-steps/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(ms, 5), "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "f32", "data": "synthetic (Philox resets; reference GoTo seed_0 weights)",
                "step": f"one training episode: reset + {max_steps} ticks", "us_per_tick": round(tick_ms * 1e3, 3),
                "tick_us": tick_spread,
                "config": {"workload": f"{scen} train tick: {N} agents x {B} envs/GPU, {args.conv.upper()}, "
                                       f"{ {'complete': 'complete', 'knn': f'kNN-{args.knn_k}', 'radius': f'radius-{args.radius}'}[args.graph]} graph, "
                                       f"eps 0.05, TD batch {S} graphs/GPU", "envs_per_gpu": B, "agents": N,
                           "global_envs": B * world, "td_batch_per_gpu": S, "graph": args.graph, "conv": args.conv,
                           "parallelism": f"env-sharded dp{world}" + ("" if not distributed else
                                          " + xGMI peer grad all-reduce" if peer is not None else
                                          f" + {'RCCL' if args.backend == 'nccl' else args.backend} grad all-reduce"),
                           "hipgraph": graph is not None, "tick": "1 launch + reduce" if fused else "3 launches",
                           "allreduce": allreduce, "allreduce_paths": both, "peer_fused_check": fused_check,
                           "rank_errors": rank_errors,
                           "replicas_identical": replicas},
                "roofline": roof, "cpu_baseline": cpu, "acting_only": acting, "build": build,
                "loss": ctrl["loss"]}
        print(json.dumps(line))
    if distributed:
        torch.distributed.destroy_process_group()


DUMP_BUDGET_BYTES = 64 << 20


def train_outputs(eng) -> dict:
    """What the last training tick left a caller of the engine: the env state, the tick's
    reward / mean goal distance / hits, the learner (the weights in use and the set the pending
    optimizer step writes, the Adam moments, the target, the reduced gradient with its loss
    sum) and the control block's loss and gradient norm.  Read as they stand (no flush)."""
    out = {"state": eng.state, "reward": eng.reward, "avg_dist": eng.avg_dist, "hits": eng.hits,
           "params": eng.params, "params_next": eng.w_nxt, "adam_m": eng.adam_m, "adam_m_next": eng.m_nxt,
           "adam_v": eng.adam_v, "adam_v_next": eng.v_nxt, "target": eng.target, "grad": eng.grad,
           "loss_gradnorm": eng.ctrl.view(torch.float32)[5:7]}
    if eng.scenario_state is not None:
        out["scenario_state"] = eng.scenario_state
    return out


def dump_outputs(where: str, arrays: dict, rank: int = 0, world: int = 1) -> None:
    """Write each array as where/<name>.npy (float32; rank r > 0 of several: <name>.rank<r>.npy).
    All files together stay under DUMP_BUDGET_BYTES: an array above its equal share of the budget
    is written as a fixed sample of its flattened elements (sorted indices from a generator seeded
    with 0, so two runs with the same arguments sample the same elements).  Called after the timed
    region's synchronize; the copies to the host wait for anything still queued."""
    os.makedirs(where, exist_ok=True)
    share = DUMP_BUDGET_BYTES // (max(1, len(arrays)) * world) // 4 - 64   # elements per file, header allowed for
    for name, t in arrays.items():
        a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
        if a.size > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(where, name + ("" if rank == 0 else f".rank{rank}") + ".npy"), a)


def lib_identity() -> dict:
    """The library this process runs: swarm_build_info() (ABI, source digest) and the .so's sha256."""
    from swarm_amd import _lib
    h = hashlib.sha256()
    with open(_lib.LIB_PATH, "rb") as f:
        h.update(f.read())
    return {"info": _lib.load().swarm_build_info().decode(), "lib_sha256": h.hexdigest()}


def find_pmc(kernel: str, build: dict) -> dict:
    """The newest PMC summary under profiles/ (tools/pmc_summary.py) for `kernel` whose recorded
    build is this library (same swarm_build_info, i.e. the same sources and flags); none -> the
    reason, and the roofline's counters stay null."""
    cands = []
    for f in os.listdir(os.path.join(ROOT, "profiles")):
        if f.endswith(".json") and "pmc" in f:
            try:
                d = json.load(open(os.path.join(ROOT, "profiles", f)))
            except ValueError:
                continue
            if isinstance(d, dict) and d.get("kernel") == kernel:
                cands.append((os.path.getmtime(os.path.join(ROOT, "profiles", f)), f, d))
    for _, f, d in sorted(cands, reverse=True):
        b = d.get("build") or {}
        if b.get("info") == build["info"]:
            return {"file": f, "match": "build_info" + (" + lib_sha256" if b.get("lib_sha256") == build["lib_sha256"]
                                                       else ""), "data": d}
    return {"file": None, "reason": f"no PMC summary of this build ({build['info']}) under profiles/"}


def host_cpu():
    """The host's CPU as the process sees it: model name (/proc/cpuinfo), os.cpu_count(), the
    CPUs this process may run on (sched_getaffinity) and the cgroup CPU quota, if any."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    n = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = n
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    return {"model": model or platform.processor() or "unknown", "os_cpu_count": n, "affinity": aff,
            "cgroup_quota_cpus": quota}


def cpu_baseline_leg(args, w0, scen, B, N, S, eng):
    """SURVEY §8(d) CPU baseline on the GPU box's host cores (after the timed region; rank 0,
    N = 1): the vectorised PyTorch-CPU oracle on a bounded sample of the same workload, at the
    thread count the process may use (affinity / cgroup quota) and at os.cpu_count() threads
    when that differs (the faster is reported: no throttled baseline); the reference-shaped
    B = 1 training loop; and BASELINE.json configs[0] (C1: GoTo, 5 agents, 1 env, the
    evaluation script's loop with kNN-5) beside this framework's GPU at that same shape."""
    from oracle import cpu_baseline
    info = host_cpu()
    usable = info["affinity"]
    if info["cgroup_quota_cpus"]:
        usable = max(1, min(usable, math.ceil(info["cgroup_quota_cpus"])))
    # os.cpu_count() threads as well, unless a cgroup quota caps the process below that: there a
    # 256-thread oracle on a 16-CPU quota ran 1 tick in 18.6 s (profiles/r03_v1_bench.json),
    # oversubscription, not a baseline
    quota_capped = info["cgroup_quota_cpus"] is not None and info["cgroup_quota_cpus"] < info["os_cpu_count"]
    counts = [usable] if quota_capped else sorted({usable, info["os_cpu_count"]})
    info["threads_rule"] = ("the cgroup CPU quota (all the CPU time this process may use)" if quota_capped else
                            "the CPUs this process may run on, and os.cpu_count()")
    sid = 0 if scen == "GoTo" else 1
    sweep = []
    for th in counts:
        torch.set_num_threads(th)
        r = cpu_baseline.vectorized_train(w0, sid, B, N, S, seconds=args.cpu_seconds)
        sweep.append({"threads": th, "value": round(r["agent_steps_per_s"], 1), "ticks": r["ticks"],
                      "seconds": round(r["seconds"], 2)})
    best = max(sweep, key=lambda x: x["value"])
    torch.set_num_threads(best["threads"])
    r1 = cpu_baseline.reference_shaped_train(w0, sid, N, seconds=max(3.0, args.cpu_seconds / 3))
    wgo = torch.tensor(np.load(os.path.join(ROOT, "tests", "golden", "weights.npz"))["weights_go_to"][0])
    c1 = cpu_baseline.reference_shaped_eval(wgo, 0, 5, 5, seconds=args.c1_seconds)
    # the same C1 shape on the GPU: one env, 5 agents, kNN-5, greedy, 50-tick episodes, each
    # episode one swarm_rollout launch
    import swarm_amd
    e1 = swarm_amd.SwarmEngine("GoTo", 5, 1, seed=0, params=wgo, graph="knn", knn_k=5, learn=False, eps=0.0)
    for i in range(3):
        e1.reset()
        e1.rollout(50, tick0=50 * i, eps=0.0)
    torch.cuda.synchronize()
    g0 = time.perf_counter()
    for i in range(40):
        e1.reset()
        e1.rollout(50, tick0=50 * i, eps=0.0)
    torch.cuda.synchronize()
    g_el = time.perf_counter() - g0
    return {"value": best["value"], "unit": "agent-steps/s", "cores": best["threads"], "kind": "port",
            "sample": f"vectorised PyTorch-CPU oracle, same workload ({B} envs x {N} agents, S={S}), "
                      f"{best['ticks']} ticks in {best['seconds']:.1f}s on {best['threads']} threads",
            "host": info, "thread_sweep": sweep,
            "reference_shaped_b1": {"value": round(r1["agent_steps_per_s"], 1), "threads": best["threads"],
                                    "sample": f"B=1 loop shaped like train_gcn_dqn.py:153-178 (S=32), "
                                              f"{r1['ticks']} ticks in {r1['seconds']:.1f}s"},
            "c1": {"config": "BASELINE.json configs[0]: GoTo, 5 agents, 1 env, CPU PyTorch reference "
                             "(tests/ script shape: simulator.py:47-109 with kNN-5, 50-tick episodes)",
                   "value": round(c1["agent_steps_per_s"], 1), "unit": "agent-steps/s",
                   "threads": best["threads"], "sample": f"{c1['ticks']} ticks in {c1['seconds']:.1f}s",
                   "gpu_same_shape": {"value": round(5 * 50 * 40 / g_el, 1), "unit": "agent-steps/s",
                                      "us_per_tick": round(g_el / (50 * 40) * 1e6, 3),
                                      "sample": "40 episodes, reset + one 50-tick swarm_rollout launch each"}}}


ACT_PMC_CONFIG = ("GoTo", 8, 1024, "knn", 5, "gat", "gcn")   # the acting line whose rollout has PMC passes


def rollout_roofline(args, eng, max_steps, f_node):
    """The rollout kernel's roofline: algorithmic FLOPs of one max_steps-tick swarm_rollout launch
    (B·N·ticks·(forward + ≈300 FLOP of physics)) ÷ that launch's duration, HIP events on its stream
    (median of 5 launches), against the FP32 peak.  For the headline acting configuration (GoTo
    8 x 1024, kNN-5) `traffic` is the launch's HBM bytes from the PMC summary of THIS build
    (tools/pmc_summary.py, kernel "rollout"), beside SURVEY §8(d)'s algorithmic 56 B per
    agent-step (state 32 + replay push 24) and the rollout's own minimum (the state read and
    written once per launch: it stays in registers across the ticks, and a rollout pushes no
    replay)."""
    B, N = args.envs, args.agents
    stream = torch.cuda.current_stream()
    per = []
    for _ in range(5):
        eng.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.rollout(max_steps, eps=0.0)
        e1.record(stream)
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e-3)
    t_l = float(np.median(per))
    flops = B * N * max_steps * f_node
    ach = flops / t_l / 1e12
    traffic, pmc = None, {"file": None, "reason": "counters are collected for the headline acting configuration only"}
    if (args.scenario, N, B, args.graph, args.knn_k, args.conv, args.net) == ACT_PMC_CONFIG:
        pmc = find_pmc("rollout", lib_identity())
        if pmc.get("file"):
            traffic = pmc.pop("data").get("hbm_bytes_per_launch")
    alg_bytes = 56 * B * N * max_steps
    return {"bound": "valu" if args.net == "gat3" else "mfma", "achieved": round(ach, 4),
            "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_FP32_TFLOPS, "traffic": traffic,
            "kernel": "act_kernel rollout (swarm_rollout)", "algorithmic_flops_per_launch": flops,
            "flops_per_agent_step": f_node, "launch_us": round(t_l * 1e6, 2),
            "algorithmic_bytes_per_launch": alg_bytes,
            # state read + written once (32 B per agent), reward sums (4) and last obs (24) per agent,
            # mean goal distance and hits per env (8)
            "rollout_minimum_bytes_per_launch": 60 * B * N + 8 * B,
            "traffic_over_algorithmic": (traffic / alg_bytes) if traffic else None,
            "hbm_gbs": round(traffic / t_l / 1e9, 2) if traffic else None, "pmc": pmc}


def acting_fnode(args, eng) -> float:
    d = mean_in_degree(args, eng)
    if args.net == "gat3":
        return gat3_fwd_flops(args.agents, d) + 300
    return (gat_fwd_flops(args.agents, d) if args.conv == "gat" else gcn_fwd_flops(args.agents, d)) + 300


def acting_leg(args, eng, max_steps, n_steps: int = 20) -> dict:
    """Acting-only rollouts on `eng` (frozen weights, eps 0): n_steps episodes of reset + one
    max_steps-tick swarm_rollout launch, host wall clock, plus the rollout kernel's roofline."""
    B, N = args.envs, args.agents

    def rollouts(n):
        for i in range(n):
            eng.reset()
            eng.rollout(max_steps, tick0=i * max_steps, eps=0.0)
    rollouts(3)
    torch.cuda.synchronize()
    a0 = time.perf_counter()
    rollouts(n_steps)
    torch.cuda.synchronize()
    a_el = time.perf_counter() - a0
    g = {"complete": "complete", "knn": f"kNN-{args.knn_k}", "radius": f"radius-{args.radius}"}[args.graph]
    out = {"value": round(B * N * n_steps * max_steps / a_el, 1), "unit": "agent-steps/s",
           "us_per_tick": round(a_el / (n_steps * max_steps) * 1e6, 3),
           "step": f"reset + {max_steps}-tick rollout launch (swarm_rollout), {n_steps} steps", "graph": g}
    if not args.no_kernel_timing:
        out["roofline"] = rollout_roofline(args, eng, max_steps, acting_fnode(args, eng))
    return out


def bench_act(args, eng, world, rank, distributed, max_steps):
    """Acting-only throughput (SURVEY §8(d) "acting-only": S = 0, frozen weights, like
    Simulator.run_simulation): graph -> GAT/GCN Q -> argmax -> env.step for every env, episodes of
    max_steps ticks, each episode ONE swarm_rollout launch (weights staged once, state kept in
    registers across ticks).  No collective: N > 1 runs independent replicas."""
    B, N = args.envs, args.agents

    def run(n_episodes):   # one step = one episode: reset, then one max_steps-tick rollout launch
        res = None
        for i in range(n_episodes):
            eng.reset()
            res = eng.rollout(max_steps, tick0=i * max_steps, eps=0.0)
        return res

    run(args.warmup)
    torch.cuda.synchronize()
    if distributed:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    last = run(args.steps)
    torch.cuda.synchronize()
    if distributed:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:   # the last timed rollout's results and the state it left
        dump_outputs(args.dump_outputs, {"state": eng.state, **(last or {})}, rank, world)
    roof = None
    if args.full and not args.no_kernel_timing:   # one 100-tick rollout launch, HIP events on its stream
        roof = rollout_roofline(args, eng, max_steps, acting_fnode(args, eng))
    if rank == 0:
        g = {"complete": "complete", "knn": f"kNN-{args.knn_k}", "radius": f"radius-{args.radius}"}[args.graph]
        line = {"metric": "env-steps/sec (agents×envs), acting-only rollout",
                "value": round(B * N * world * args.steps * max_steps / elapsed, 1),
                "unit": "agent-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1e3, 5), "higher_is_better": True, "scaling": "weak",
                "step": f"one episode: reset + {max_steps}-tick rollout launch",
                "vs_baseline": None, "dtype": "f32", "data": "synthetic (Philox resets; reference seed_0 weights)",
                "config": {"workload": f"{args.scenario} acting-only: {N} agents x {B} envs/GPU, "
                                       f"{'GAT3 (Flocking checkpoints)' if args.net == 'gat3' else args.conv.upper()}, "
                                       f"{g} graph, eps 0, frozen weights", "envs_per_gpu": B, "agents": N,
                           "global_envs": B * world, "graph": args.graph, "conv": args.conv,
                           "parallelism": f"replicas x{world}"},
                "roofline": roof, "cpu_baseline": None, "build": lib_identity()}
        print(json.dumps(line))
    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
