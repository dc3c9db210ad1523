"""Bit-for-bit comparison of two builds of libswarm_hip.so on the same seeded work.

Each library runs in its own child process (SWARM_LIB_PATH; "base" = the in-tree library), which
runs a list of cases and saves every output; the parent reports, one JSON line per case, whether
the two runs agree bit for bit (a kernel change meant to move only code, stores or schedules must
leave every bit alone).  The kinds of case:
  tick : a fused engine (batch = envs) is prefilled with 3 acting ticks, then runs `ticks` training
         ticks; the gradient after every tick and the final weights, Adam moments, target and
         control block;
  td   : the unfused swarm_td_grad on a seeded replay (tests/test_gpu_parity.py _fill_replay) and a
         fixed sample_in; the gradient buffer;
  qb   : swarm_q_backward on a case of tests/test_q_backward.py; the whole gradient buffer;
  g3b  : swarm_gat3_q_backward on a case of tests/test_gat3_backward.py; its 416-float gradient buffer;
  g3t  : a SwarmGat3Engine (swarm_act_step, swarm_gat3_td_grad, swarm_gat3_adam_step) runs `ticks` training
         ticks; the gradient and the batch indices after every tick and the final weights, Adam moments,
         target, ring, state and control block.

usage: python tools/bitcmp.py LIB_A LIB_B [scenario N B ticks]    one tick case (LIB = base or a path)
       python tools/bitcmp.py LIB_A LIB_B --matrix [OUT.jsonl] [--kinds=g3t,g3b]   MATRIX: every instance of
           the TD kernel, the fused tick and q_backward at its smallest size, then the benchmark's sizes
           (--kinds: only its cases of these kinds)
Exit status 1 when a case differs or a run counted a hand-off error.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kind, ...): tick: scenario, N, envs, ticks, graph, conv; td: scenario, N, S, graph, k, conv; qb, g3b: case index;
# g3t: N, envs, batch, ring, ticks, graph, k
MATRIX = (
    [("tick", scen, N, B, 6, "complete", conv)
     for scen, N, B in (("GoTo", 5, 64),                 # two 8-slot graphs per wave, padded slots
                        ("GoTo", 8, 64), ("ObstacleAvoidance", 12, 64), ("ObstacleAvoidance", 16, 32), ("Flocking", 8, 64))
     for conv in ("gat", "gcn")]
    + [("tick", "GoTo", 8, 64, 6, "radius", "gat")]      # the runtime-graph tick instance
    # the 32-slot TD instances (two column tiles; no fused tick has them) and the runtime-graph one
    + [("td", "ObstacleAvoidance", N, 5, "complete", 0, conv) for N in (20, 29) for conv in ("gat", "gcn")]
    + [("td", "ObstacleAvoidance", 12, 5, "knn", 5, "gat")]
    + [("qb", i) for i in range(17)]
    + [("g3b", i) for i in range(13)]                    # every slot class, graph kind and the two-slab reduce groups
    # the three-layer GAT's learner: every slot class and graph kind, skipped ticks, a wrapping ring
    + [("g3t", 5, 2, 7, 8, 10, "complete", 0), ("g3t", 12, 5, 5, 10, 8, "knn", 5), ("g3t", 17, 2, 3, 4, 6, "radius", 0),
       ("g3t", 10, 1, 32, 1000, 36, "complete", 0)]
    + [("tick", scen, N, B, 6, "complete", "gat")        # the benchmark's sizes
       for scen, N, B in (("GoTo", 8, 1024), ("ObstacleAvoidance", 12, 1024), ("ObstacleAvoidance", 5, 512),
                          ("ObstacleAvoidance", 12, 512))]
)


def run_case(case):
    """the outputs of one case on the library this process loaded: {name: CPU tensor} and the hand-off errors"""
    import numpy as np
    import torch
    import swarm_amd
    golden = np.load(os.path.join(ROOT, "tests", "golden", "weights.npz"))
    kind = case[0]
    if kind == "tick":
        _, scen, N, B, T, graph, conv = case
        w0 = torch.tensor(golden["weights_go_to" if scen == "GoTo" else "weights_obstacle_avoidance"][0])
        eng = swarm_amd.SwarmEngine(scen, N, B, seed=3, params=w0, batch=B, eps=0.2, replay_capacity=8 * B,
                                    update_target_every=3, graph=graph, conv=conv)
        assert eng.fused
        eng.reset(0)
        for _ in range(3):
            eng.act(push=True, full_out=False)
            eng.advance()
        grads = []
        for t in range(T):
            eng.train_tick()
            torch.cuda.synchronize()
            grads.append(eng.grad.cpu().clone())
        eng.flush()
        torch.cuda.synchronize()
        return {"grads": torch.stack(grads), "params": eng.params.cpu(), "m": eng.adam_m.cpu(), "v": eng.adam_v.cpu(),
                "target": eng.target.cpu(), "ctrl": eng.ctrl.cpu()}, eng.handoff_errors()
    if kind == "td":
        from tests.test_gpu_parity import _fill_replay
        _, scen, N, S, graph, k, conv = case
        B, cap = 16, 4
        w = golden["weights_obstacle_avoidance"]
        eng = swarm_amd.SwarmEngine(scen, N, B, seed=2, params=torch.tensor(w[5]), batch=S, replay_capacity=cap * B,
                                    update_target_every=1000, graph=graph, knn_k=max(k, 1), conv=conv, radius=0.5)
        eng.target.copy_(torch.tensor(w[6]).cuda())
        _fill_replay(eng, S)
        idx = torch.randperm(cap * B, generator=torch.Generator().manual_seed(S))[:S].to(torch.int32)
        eng.td_grad(sample_in=idx.cuda())
        torch.cuda.synchronize()
        return {"grad": eng.grad.cpu()}, eng.handoff_errors()
    if kind == "g3t":
        _, N, B, S, ring, T, graph, k = case
        eng = swarm_amd.SwarmGat3Engine("Flocking", N, B, seed=3, batch=S, eps=0.3, replay_capacity=ring,
                                        update_target_every=3, graph=graph, knn_k=max(k, 1), radius=0.5)
        eng.reset(0)
        grads, samples = [], []
        for t in range(T):
            eng.train_tick(full_out=True)
            grads.append(eng.grad.clone())
            samples.append(eng.samples.clone())
        torch.cuda.synchronize()
        assert eng.read_ctrl()["adam_step"] >= 1
        out = {k: getattr(eng, k).cpu() for k in ("params", "adam_m", "adam_v", "target", "rep_s", "rep_s1", "rep_r",
                                                  "rep_a", "_state_buf", "ctrl", "q")}
        return dict(out, grad=torch.stack(grads).cpu(), samples=torch.stack(samples).cpu()), 0
    if kind == "g3b":
        from tests import test_gat3_backward as T
        N, B, graph, k, seed, holes = T.CASES[case[1]]
        s, x, mult, dq = T._case_inputs(N, B, graph, k, holes)
        p = torch.tensor(np.load(os.path.join(ROOT, "tests", "golden", "flocking_weights.npz"))["weights_flocking"][seed])
        return {"grad": T._Call(N, B, graph, k, p, x, mult, dq).run()}, 0
    from tests.test_q_backward import CASES, _case_inputs, _q_backward
    scen, N, B, graph, k, conv, holes = CASES[case[1]]
    s, x, mult, dq = _case_inputs(N, B, graph, k, holes)
    p = torch.tensor(golden["weights_" + scen][5])
    return {"grad": _q_backward(scen, N, B, graph, k, conv, p, x, mult, dq)}, 0


def child(out, cases):
    import torch
    sys.path.insert(0, ROOT)
    import swarm_amd
    res = []
    for case in cases:
        tensors, ho = run_case(case)
        res.append({"tensors": tensors, "ho": ho})
    torch.save({"cases": res, "build": swarm_amd._lib.load().swarm_build_info().decode()}, out)


def run(lib, cases, out):
    env = dict(os.environ)
    if lib != "base":
        env["SWARM_LIB_PATH"] = os.path.abspath(lib)
    else:
        env.pop("SWARM_LIB_PATH", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, json.dumps(cases)], env=env, check=True,
                   timeout=600)


def same_bits(x, y):
    import torch
    return x.shape == y.shape and x.dtype == y.dtype and bool(torch.equal(x.contiguous().view(torch.uint8),
                                                                          y.contiguous().view(torch.uint8)))


def main():
    import torch
    if sys.argv[1] == "--child":
        return child(sys.argv[2], [tuple(c) for c in json.loads(sys.argv[3])])
    a, b = sys.argv[1], sys.argv[2]
    log = None
    kinds = [x[len("--kinds="):].split(",") for x in sys.argv if x.startswith("--kinds=")]
    sys.argv = [x for x in sys.argv if not x.startswith("--kinds=")]
    if len(sys.argv) > 3 and sys.argv[3] == "--matrix":
        cases, log = MATRIX, sys.argv[4] if len(sys.argv) > 4 else None
        if kinds:
            cases = [c for c in MATRIX if c[0] in kinds[0]]
    else:
        scen = sys.argv[3] if len(sys.argv) > 3 else "GoTo"
        N = int(sys.argv[4]) if len(sys.argv) > 4 else 8
        B = int(sys.argv[5]) if len(sys.argv) > 5 else 1024
        T = int(sys.argv[6]) if len(sys.argv) > 6 else 6
        cases = [("tick", scen, N, B, T, "complete", "gat")]
    with tempfile.TemporaryDirectory() as d:
        pa, pb = os.path.join(d, "a.pt"), os.path.join(d, "b.pt")
        run(a, cases, pa)
        run(b, cases, pb)
        ra, rb = torch.load(pa, weights_only=True), torch.load(pb, weights_only=True)
    ok, equal, lines = True, 0, []
    for case, ca, cb in zip(cases, ra["cases"], rb["cases"]):
        res = {"a": a, "b": b, "build_a": ra["build"], "build_b": rb["build"], "config": list(case),
               "handoff_errors": [ca["ho"], cb["ho"]]}
        for k in ca["tensors"]:
            res[k + "_bitwise"] = same_bits(ca["tensors"][k], cb["tensors"][k])
        res["all_bitwise"] = all(res[k + "_bitwise"] for k in ca["tensors"])
        g = "grads" if case[0] == "tick" else "grad"
        res["grad_max_abs_diff"] = float((ca["tensors"][g] - cb["tensors"][g]).abs().nan_to_num(0.0).max())
        equal += res["all_bitwise"]
        ok = ok and res["all_bitwise"] and ca["ho"] == 0 and cb["ho"] == 0
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(f"{equal} of {len(lines)} cases bitwise equal")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
