"""CPU-only tests of the host side of the three-layer GAT's learner entry points
(swarm_gat3_td_grad, swarm_gat3_adam_step): what they return before they would launch anything, their
declarations, the slab bound of the batch-sized workspace, ``glorot_init``'s ``net`` argument and
the keywords of the classes on top.  No GPU compute is called here."""
import ctypes
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (what, config overrides, hp overrides, NULL argument or None, expected code), in the entry points'
# order of checks: every call is rejected, so 1 can stand in for every device pointer.
# Base: 8 agents, 16 envs, Flocking, complete graph, GAT, the three-layer net; batch 4, world size 1.
_BASE = dict(B=16, N=8, scen=2, graph=0, k=0, conv=0, radius=0.0, net=1)
_HP = dict(batch=4, every=200, world=1)
_CONFIG = (
    # 1. the configuration and hp, as swarm_td_grad / swarm_adam_step check them
    ("cfg NULL", {}, {}, "cfg", -1),
    ("hp NULL", {}, {}, "hp", -1),
    ("N = 0", {"N": 0}, {}, None, -1),
    ("N = 33", {"N": 33}, {}, None, -1),
    ("B = 0", {"B": 0}, {}, None, -1),
    ("batch = 0", {}, {"batch": 0}, None, -1),
    ("batch = 0, net GCN", {"net": 0}, {"batch": 0}, None, -1),
    ("graph 4", {"graph": 4}, {}, None, -1),
    ("GAT3 with GCNConv", {"conv": 1}, {}, None, -1),
    ("net 2", {"net": 2}, {}, None, -1),
    ("kNN k = 0", {"graph": 1, "k": 0}, {}, None, -2),
    ("kNN k = N + 1", {"graph": 1, "k": 9}, {}, None, -2),
    ("net GCN, kNN k = 0", {"net": 0, "graph": 1, "k": 0}, {}, None, -2),   # the config is checked before the net
    ("radius 0", {"graph": 3}, {}, None, -1),
    ("update_target_every = 0", {}, {"every": 0}, None, -1),
    ("update_target_every = 0, net GCN", {"net": 0}, {"every": 0}, None, -1),
    ("world_size = 0", {}, {"world": 0}, None, -1),
    # 2. the net
    ("net GCN", {"net": 0}, {}, None, -4),
    ("net GCN with GCNConv", {"net": 0, "conv": 1}, {}, None, -4),
    ("net GCN, world_size = 2", {"net": 0}, {"world": 2}, None, -4),
    ("net GCN, dense graph", {"net": 0, "graph": 2}, {}, None, -4),
    ("net GCN, params NULL", {"net": 0}, {}, "params", -4),
    # 3. the world size
    ("world_size = 2", {}, {"world": 2}, None, -4),
    ("world_size = 2, dense graph", {"graph": 2}, {"world": 2}, None, -4),
    ("world_size = 2, grad NULL", {}, {"world": 2}, "grad", -4),
    # 4. the dense graph
    ("dense graph", {"graph": 2}, {}, None, -1),
)
# 5. the pointers and the capacity, per entry point
_TD_NULLS = ("params", "target", "replay", "ctrl", "workspace", "grad",
             "replay.s", "replay.s_next", "replay.r", "replay.a", "capacity")
_ADAM_NULLS = ("params", "target", "adam_m", "adam_v", "grad", "ctrl", "capacity")


def _host_lib():
    import swarm_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load(require_gpu=False)


def _cfg_hp(L, over, hp_over):
    c, h = dict(_BASE, **over), dict(_HP, **hp_over)
    cfg = L.SwarmConfig(c["B"], c["N"], c["scen"], c["graph"], c["k"], c["conv"], 0, 0, 7, c["radius"], c["net"])
    hp = L.SwarmAdamCfg(1e-3, 0.9, 0.999, 1e-8, 1.0, 0.99, h["batch"], h["every"], h["world"], 0, 1e-3, 0.9, 0.999)
    return cfg, hp


def _td(L, lib, over, hp_over, null):
    cfg, hp = _cfg_hp(L, over, hp_over)
    rp = {n: (0 if null == "replay." + n else 1) for n in ("s", "s_next", "r", "a")}
    rep = L.SwarmReplay(rp["s"], rp["s_next"], rp["r"], rp["a"], 0 if null == "capacity" else 4, 0)
    P = {n: (None if n == null else 1) for n in ("params", "target", "ctrl", "workspace", "grad")}
    return lib.swarm_gat3_td_grad(None if null == "cfg" else ctypes.byref(cfg), None if null == "hp" else ctypes.byref(hp),
                                  P["params"], P["target"], None if null == "replay" else ctypes.byref(rep), P["ctrl"],
                                  None, None, P["workspace"], P["grad"], None)


def _adam(L, lib, over, hp_over, null):
    cfg, hp = _cfg_hp(L, over, hp_over)
    P = {n: (None if n == null else 1) for n in ("params", "target", "adam_m", "adam_v", "grad", "ctrl")}
    return lib.swarm_gat3_adam_step(None if null == "cfg" else ctypes.byref(cfg),
                                    None if null == "hp" else ctypes.byref(hp), P["params"], P["target"], P["adam_m"],
                                    P["adam_v"], P["grad"], 0 if null == "capacity" else 4, P["ctrl"], None)


def test_gat3_td_grad_error_codes_are_pinned():
    L, lib = _host_lib()
    for what, over, hp_over, null, code in _CONFIG:
        assert _td(L, lib, over, hp_over, null) == code, what
    for null in _TD_NULLS:
        assert _td(L, lib, {}, {}, null) == -1, null
        assert _td(L, lib, {"N": 32, "graph": 3, "radius": 0.5}, {}, null) == -1, null


def test_gat3_adam_step_error_codes_are_pinned():
    L, lib = _host_lib()
    for what, over, hp_over, null, code in _CONFIG:
        if null in (None, "cfg", "hp", "params", "grad"):
            assert _adam(L, lib, over, hp_over, null) == code, what
    for null in _ADAM_NULLS:
        assert _adam(L, lib, {}, {}, null) == -1, null


def test_closed_doors_stay_closed():
    """The one-layer network's learner entry points still refuse the three-layer net."""
    import swarm_amd
    L, lib = _host_lib()
    cfg, hp = _cfg_hp(L, {}, {})
    rep = L.SwarmReplay(1, 1, 1, 1, 4, 0)
    assert lib.swarm_td_grad(ctypes.byref(cfg), ctypes.byref(hp), 1, 1, ctypes.byref(rep), 1, None, None, 1, None) == -4
    assert lib.swarm_adam_step(ctypes.byref(cfg), ctypes.byref(hp), 1, 1, 1, 1, 1, 4, 1, None) == -4
    assert lib.swarm_q_backward(ctypes.byref(cfg), 1, 1, None, 1, 1, 1, None) == -4
    assert lib.swarm_train_tick_supported(ctypes.byref(cfg)) == 0
    with pytest.raises(ValueError, match="GAT3"):
        swarm_amd.GCN(7, 8, 9, layers=3, autograd=True)
    assert swarm_amd.SwarmEngine.trains_gat3 is False and swarm_amd.SwarmGat3Engine.trains_gat3 is True


def test_entry_points_are_declared_everywhere():
    L, lib = _host_lib()
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("swarm_gat3_td_grad", "swarm_gat3_adam_step"):
        assert name in L.EXPORTED and name in L._NEWEST and hasattr(lib, name)
        assert f"int {name}(" in hdr
        assert f"`{name}" in doc
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10 and "#define SWARM_ABI_VERSION 10" in hdr


def test_td_slabs_fit_the_batch_sized_workspace():
    """The TD kernel writes one 416-float slab per block of sampled graphs into the workspace the
    caller sized with swarm_td_workspace_floats(cfg, hp->batch)."""
    from swarm_amd.graph import gat3_backward_slab_floats
    L, lib = _host_lib()
    for N in (2, 8, 9, 16, 17, 32):
        for S in (1, 4, 5, 32, 260, 1024):
            cfg = L.SwarmConfig(16, N, 2, 0, 0, 0, 0, 0, 0, 0.0, L.NET_GAT3)
            have = lib.swarm_td_workspace_floats(ctypes.byref(cfg), S)
            assert have >= gat3_backward_slab_floats(N, S), (N, S, have)


def _old_glorot_init(generator):
    """engine.glorot_init as it was before it took ``net``."""
    from swarm_amd.engine import flatten_state_dict

    def glorot(shape, fan_in, fan_out):
        a = math.sqrt(6.0 / (fan_in + fan_out))
        return (torch.rand(shape, generator=generator) * 2 - 1) * a

    def linear(out_f, in_f):
        b = 1.0 / math.sqrt(in_f)
        w = (torch.rand(out_f, in_f, generator=generator) * 2 - 1) * b
        bias = (torch.rand(out_f, generator=generator) * 2 - 1) * b
        return w, bias

    sd = {
        "conv1.att_src": glorot((1, 1, 32), 1, 32),
        "conv1.att_dst": glorot((1, 1, 32), 1, 32),
        "conv1.bias": torch.zeros(32),
        "conv1.lin.weight": glorot((32, 7), 7, 32),
    }
    sd["lin1.weight"], sd["lin1.bias"] = linear(32, 32)
    sd["lin2.weight"], sd["lin2.bias"] = linear(9, 32)
    return flatten_state_dict(sd)


def test_glorot_init_default_is_unchanged_and_gat3_follows_its_rules():
    from swarm_amd.engine import PARAM_ORDER_GAT3, glorot_init, unflatten_params
    for seed in (0, 3, 12345):
        old = _old_glorot_init(torch.Generator().manual_seed(seed))
        new = glorot_init(torch.Generator().manual_seed(seed))
        assert old.shape == (1673,) and torch.equal(old, new)
        assert torch.equal(old, glorot_init(torch.Generator().manual_seed(seed), "gcn"))
    flat = glorot_init(torch.Generator().manual_seed(3), "gat3")
    assert flat.shape == (409,) and flat.dtype == torch.float32 and torch.isfinite(flat).all()
    assert torch.equal(flat, glorot_init(torch.Generator().manual_seed(3), net="gat3"))
    sd = unflatten_params(flat, "gat3")
    assert list(sd) == [k for k, _ in PARAM_ORDER_GAT3]
    for i, k in ((1, 7), (2, 8), (3, 8)):
        assert not sd[f"conv{i}.bias"].any()
        assert sd[f"conv{i}.lin.weight"].abs().max() <= math.sqrt(6.0 / (k + 8)) and sd[f"conv{i}.lin.weight"].any()
        for att in ("att_src", "att_dst"):
            assert sd[f"conv{i}.{att}"].abs().max() <= math.sqrt(6.0 / 9) and sd[f"conv{i}.{att}"].any()
    for k in ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"):
        assert sd[k].abs().max() <= 1.0 / math.sqrt(8) and sd[k].any()


def test_class_keywords():
    import importlib
    import sys
    import swarm_amd
    from swarm_amd.dqn import DQNTrainer
    sys.path.insert(0, os.path.join(ROOT, "compat", "src", "training"))   # as the reference's scripts import it
    try:
        compat = importlib.import_module("train_gcn_dqn")
    finally:
        sys.path.pop(0)
        sys.modules.pop("train_gcn_dqn", None)
    assert compat.SwarmGat3Engine is swarm_amd.SwarmGat3Engine
    assert "SwarmGat3Engine" in swarm_amd.__all__ and "SwarmGat3Engine" in compat.__all__
    assert issubclass(swarm_amd.SwarmGat3Engine, swarm_amd.SwarmEngine)
    eng = swarm_amd.SwarmGat3Engine
    assert eng.train_tick3 is eng.launch_tick is eng.launch_train_act
    with pytest.raises(ValueError, match="unfused"):
        eng.train_tick3(None)
    import inspect
    assert inspect.signature(DQNTrainer.__init__).parameters["net"].default == "gcn"
