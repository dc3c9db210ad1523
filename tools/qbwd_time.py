"""Time swarm_q_backward against the TD pair it shares its second launch with.

Two chains of back-to-back launches on one stream, each between two HIP events (no host
synchronisation inside a chain, so the launch-bound kernels overlap their launches as they do in a
captured tick):
  q_backward : swarm_q_backward                       (backward kernel + slab reduce)
  td pair    : swarm_td_grad + swarm_grad_reduce      (TD kernel, in-kernel sampling + slab reduce)
at S = B graphs of N agents, complete graph, GAT.  The chains alternate, `--repeats` times each, after
a warm-up of both; the table gives the median and the spread of the per-call time of each chain.

`--net gat3` times the three-layer network's pair instead, at Flocking 8 x 1024 graphs, complete graph:
  gat3_q_backward : swarm_gat3_q_backward             (backward kernel + its slab reduce)
  gat3_q_forward  : swarm_q_forward with SWARM_NET_GAT3  (one launch; the forward of the same graphs)
on the Flocking fixture's weights of seed 4.  A record, not a gate: nothing comparable existed before.

`--net gat3-td` times the three-layer network's learner (swarm_gat3_td.h) at Flocking 8 agents x 1,024 envs,
complete graph, batch 32 and batch 1,024, and beside it, in the same run, what it is read against:
  gat3_td_grad    : swarm_gat3_td_grad                (TD kernel, in-kernel sampling + slab sum)
  gat3_adam_step  : swarm_gat3_adam_step              (one launch; lr = 0, so the weights stay put)
  gat3_tick       : SwarmGat3Engine.train_tick        (swarm_act_step + the three launches above)
  gat3_q_backward, gat3_q_forward : the parent's kernels at `batch` graphs; the work the TD kernel
                    fuses is one backward and two forwards (separate_us = backward + 2 forward)
  torch_step      : GAT3(autograd=True), torch's MSELoss, clip_grad_norm_ and Adam on the same batch
                    (the only way to do this update without the learner); calls / 20 per chain
A record, not a gate.

usage: python tools/qbwd_time.py [--net gcn|gat3|gat3-td] [--calls 2000] [--repeats 7] [--out qbwd_time.json]
Prints one JSON line per configuration.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swarm_amd  # noqa: E402
import swarm_amd._lib as L  # noqa: E402

CONFIGS = (("GoTo", 8, 1024), ("ObstacleAvoidance", 12, 1024))
GAT3_CONFIGS = (("Flocking", 8, 1024),)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def alternate(chains, calls, repeats, out):
    """Warm both chains up, alternate them `repeats` times; medians and spreads into `out`."""
    for fn in chains.values():   # warm-up: code objects loaded, clocks up
        chain_us(fn, max(calls // 4, 10))
    times = {k: [] for k in chains}
    for _ in range(repeats):
        for k, fn in chains.items():
            times[k].append(chain_us(fn, calls))
    for k, v in times.items():
        out[k + "_us"] = round(statistics.median(v), 3)
        out[k + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
    return out


def measure_gat3(scen, N, S, calls, repeats):
    import numpy as np
    lib = L.load()
    w = np.load(os.path.join(ROOT, "tests", "golden", "flocking_weights.npz"))["weights_flocking"][4]
    params = torch.tensor(w).cuda()
    g = torch.Generator().manual_seed(N)
    s = (torch.randn(S, N, 4, generator=g) * 0.4).cuda()
    ids = torch.arange(N, dtype=torch.float32, device="cuda").view(1, N, 1).expand(S, N, 1)
    goal = torch.tensor([-0.8, 0.8], device="cuda").expand(S, N, 2)
    x = torch.cat([s, goal, ids], dim=-1).reshape(S * N, 7).contiguous()
    dq = torch.randn(S * N, 9, generator=g).cuda()
    cfg = L.SwarmConfig(S, N, L.SWARM_FLOCKING, L.GRAPH_COMPLETE, 0, L.CONV_GAT, 0, 0, 0, 0.0, L.NET_GAT3)
    ws = torch.empty(lib.swarm_td_workspace_floats(ctypes.byref(cfg), S), dtype=torch.float32, device="cuda")
    grad = torch.empty(L.GAT3_GRAD_FLOATS, dtype=torch.float32, device="cuda")
    q = torch.empty(S * N, 9, dtype=torch.float32, device="cuda")
    st = L.stream_ptr()
    bargs = (ctypes.byref(cfg), L.ptr(params), L.ptr(x), None, L.ptr(dq), L.ptr(ws), L.ptr(grad), st)
    fargs = (ctypes.byref(cfg), L.ptr(params), L.ptr(x), None, L.ptr(q), st)

    def qb():
        L.check(lib.swarm_gat3_q_backward(*bargs), "swarm_gat3_q_backward")

    def qf():
        L.check(lib.swarm_q_forward(*fargs), "swarm_q_forward")

    out = {"net": "gat3", "scenario": scen, "n_agents": N, "graphs": S, "calls_per_chain": calls, "repeats": repeats,
           "build": lib.swarm_build_info().decode()}
    alternate({"gat3_q_backward": qb, "gat3_q_forward": qf}, calls, repeats, out)
    out["ratio"] = round(out["gat3_q_backward_us"] / out["gat3_q_forward_us"], 3)
    return out


def _gat3_q_pair(lib, params, N, S, g):
    """(backward, forward) calls of the parent's kernels on S random graphs of N agents"""
    s = (torch.randn(S, N, 4, generator=g) * 0.4).cuda()
    ids = torch.arange(N, dtype=torch.float32, device="cuda").view(1, N, 1).expand(S, N, 1)
    goal = torch.tensor([-0.8, 0.8], device="cuda").expand(S, N, 2)
    x = torch.cat([s, goal, ids], dim=-1).reshape(S * N, 7).contiguous()
    dq = torch.randn(S * N, 9, generator=g).cuda()
    cfg = L.SwarmConfig(S, N, L.SWARM_FLOCKING, L.GRAPH_COMPLETE, 0, L.CONV_GAT, 0, 0, 0, 0.0, L.NET_GAT3)
    ws = torch.empty(lib.swarm_td_workspace_floats(ctypes.byref(cfg), S), dtype=torch.float32, device="cuda")
    grad = torch.empty(L.GAT3_GRAD_FLOATS, dtype=torch.float32, device="cuda")
    q = torch.empty(S * N, 9, dtype=torch.float32, device="cuda")
    keep = (cfg, x, dq, ws, grad, q)   # the closures' buffers
    st = L.stream_ptr()
    bargs = (ctypes.byref(cfg), L.ptr(params), L.ptr(x), None, L.ptr(dq), L.ptr(ws), L.ptr(grad), st)
    fargs = (ctypes.byref(cfg), L.ptr(params), L.ptr(x), None, L.ptr(q), st)

    def qb(keep=keep):
        L.check(lib.swarm_gat3_q_backward(*bargs), "swarm_gat3_q_backward")

    def qf(keep=keep):
        L.check(lib.swarm_q_forward(*fargs), "swarm_q_forward")
    return qb, qf


def measure_gat3_td(scen, N, B, batch, calls, repeats):
    import numpy as np
    lib = L.load()
    w = np.load(os.path.join(ROOT, "tests", "golden", "flocking_weights.npz"))["weights_flocking"]
    p, tgt = torch.tensor(w[4]), torch.tensor(w[8])
    cap = 2
    g = torch.Generator().manual_seed(N)
    ring = ((torch.randn(cap, B, N, 4, generator=g) * 0.4), torch.randn(cap, B, N, 4, generator=g) * 0.05,
            torch.randn(cap, B, N, generator=g), torch.randint(0, 9, (cap, B, N), generator=g).to(torch.uint8))

    def engine():   # lr = 0: every launch does its whole work and the weights stay where they are
        e = swarm_amd.SwarmGat3Engine(scen, N, B, seed=1, params=p, batch=batch, replay_capacity=cap * B, lr=0.0,
                                      update_target_every=1000)
        e.target.copy_(tgt.cuda())
        e.rep_s.copy_(ring[0].cuda())
        e.rep_s1.copy_((ring[0] + ring[1]).cuda())
        e.rep_r.copy_(ring[2].cuda())
        e.rep_a.copy_(ring[3].cuda())
        e.ctrl[2] = cap
        e.reset(0)
        return e
    e_td, e_adam, e_tick = engine(), engine(), engine()
    e_adam.td_grad()
    qb, qf = _gat3_q_pair(lib, e_td.params, N, batch, g)

    # the torch route on the same batch (tests/test_gat3_backward.py's training step)
    model, target_model = swarm_amd.GAT3(autograd=True), swarm_amd.GAT3()
    model.load_state_dict(swarm_amd.unflatten_params(p, "gat3"))
    target_model.load_state_dict(swarm_amd.unflatten_params(tgt, "gat3"))
    goal = torch.tensor([-0.8, 0.8]).expand(batch, N, 2)
    s, s1 = ring[0][0, :batch], (ring[0] + ring[1])[0, :batch]
    obs = swarm_amd.create_graph_from_observations(torch.cat([s, goal], dim=-1))
    next_obs = swarm_amd.create_graph_from_observations(torch.cat([s1, goal], dim=-1))
    actions = ring[3][0, :batch].reshape(-1, 1).long().cuda()
    rewards = ring[2][0, :batch].reshape(-1).cuda()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.0)

    def torch_step():
        optimizer.zero_grad()
        values = model(obs).gather(1, actions)
        with torch.no_grad():
            next_values = target_model(next_obs).max(dim=1)[0]
        loss = torch.nn.MSELoss()(values, (rewards + 0.99 * next_values).unsqueeze(1))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
        optimizer.step()

    out = {"net": "gat3", "scenario": scen, "n_agents": N, "envs": B, "batch": batch, "calls_per_chain": calls,
           "repeats": repeats, "build": lib.swarm_build_info().decode()}
    alternate({"gat3_td_grad": e_td.td_grad, "gat3_adam_step": e_adam.adam, "gat3_tick": e_tick.train_tick,
               "gat3_q_backward": qb, "gat3_q_forward": qf}, calls, repeats, out)
    alternate({"torch_step": torch_step}, max(calls // 20, 10), repeats, out)
    assert e_tick.read_ctrl()["adam_step"] > 0 and torch.isfinite(e_td.grad[:410]).all()
    out["separate_us"] = round(out["gat3_q_backward_us"] + 2 * out["gat3_q_forward_us"], 3)
    out["td_grad_over_separate"] = round(out["gat3_td_grad_us"] / out["separate_us"], 3)
    out["torch_step_over_td_update"] = round(out["torch_step_us"] / (out["gat3_td_grad_us"] + out["gat3_adam_step_us"]), 1)
    return out


def measure(scen, N, S, calls, repeats):
    lib = L.load()
    cap = 2
    eng = swarm_amd.SwarmEngine(scen, N, S, seed=1, batch=S, replay_capacity=cap * S, update_target_every=1000,
                                graph="complete", conv="gat")
    g = torch.Generator().manual_seed(N)
    eng.rep_s.copy_((torch.randn(cap, S, N, 4, generator=g) * 0.4).cuda())
    eng.rep_s1.copy_((torch.randn(cap, S, N, 4, generator=g) * 0.4).cuda())
    eng.rep_r.copy_(torch.randn(cap, S, N, generator=g).cuda())
    eng.rep_a.copy_(torch.randint(0, 9, (cap, S, N), generator=g).to(torch.uint8).cuda())
    eng.ctrl[2] = cap
    eng.ctrl[1] = 0
    s = eng.rep_s[0]
    ids = torch.arange(N, dtype=torch.float32, device="cuda").view(1, N, 1).expand(S, N, 1)
    goal = torch.tensor([-0.8, 0.8], device="cuda").expand(S, N, 2)
    x = torch.cat([s, goal, ids], dim=-1).reshape(S * N, 7).contiguous()
    dq = torch.randn(S * N, 9, generator=g).cuda()
    cfg = L.SwarmConfig(S, N, eng.scenario_id, L.GRAPH_COMPLETE, 0, L.CONV_GAT, 0, 0, 0, 0.0, L.NET_GCN)
    ws = torch.empty(lib.swarm_td_workspace_floats(ctypes.byref(cfg), S), dtype=torch.float32, device="cuda")
    grad = torch.empty(L.GRAD_FLOATS, dtype=torch.float32, device="cuda")
    st = L.stream_ptr()
    args = (ctypes.byref(cfg), L.ptr(eng.params), L.ptr(x), None, L.ptr(dq), L.ptr(ws), L.ptr(grad), st)

    def qb():
        L.check(lib.swarm_q_backward(*args), "swarm_q_backward")

    out = {"scenario": scen, "n_agents": N, "graphs": S, "calls_per_chain": calls, "repeats": repeats,
           "build": lib.swarm_build_info().decode()}
    alternate({"q_backward": qb, "td_pair": eng.td_grad}, calls, repeats, out)
    out["ratio"] = round(out["q_backward_us"] / out["td_pair_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--net", choices=("gcn", "gat3", "gat3-td"), default="gcn")
    a = ap.parse_args()
    if a.net == "gat3-td":
        rows = [measure_gat3_td("Flocking", 8, 1024, batch, a.calls, a.repeats) for batch in (32, 1024)]
    elif a.net == "gat3":
        rows = [measure_gat3(scen, N, S, a.calls, a.repeats) for scen, N, S in GAT3_CONFIGS]
    else:
        rows = [measure(scen, N, S, a.calls, a.repeats) for scen, N, S in CONFIGS]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
