"""CPU-only tests of the host side of the GAT3 population entry points (swarm_pop_gat3_act_step,
swarm_pop_gat3_td_grad, swarm_pop_gat3_adam_step): what they return before they would launch
anything, in the header's order; the layout of swarm_gat3_member against the header; and the names
the classes on top are exported under.  No GPU compute is called here."""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Base: 8 agents, 16 envs, Flocking, complete graph, GAT, the three-layer net; batch 4, world size 1.
_BASE = dict(B=16, N=8, scen=2, graph=0, k=0, conv=0, radius=0.0, net=1)
_HP = dict(batch=4, every=200, world=1)
# (what, config overrides, hp overrides, NULL argument or None, n_members, expected code), in the
# order of the checks.  Every call is rejected, so 1 can stand in for the device tables.
_FIRST = (
    # 1. NULL arguments and the member count, before anything of the configuration is looked at
    ("cfg NULL", {}, {}, "cfg", 3, -1),
    ("members NULL", {}, {}, "members", 3, -1),
    ("members NULL, net GCN", {"net": 0}, {}, "members", 3, -1),
    ("members NULL, kNN k = 0", {"graph": 1, "k": 0}, {}, "members", 3, -1),
    ("n_members = 0", {}, {}, None, 0, -1),
    ("n_members = -1", {}, {}, None, -1, -1),
    ("n_members = 65536", {}, {}, None, 65536, -1),
    ("n_members = 0, net GCN", {"net": 0}, {}, None, 0, -1),
    ("n_members = 65536, kNN k = 0", {"graph": 1, "k": 0}, {}, None, 65536, -1),
)
_HP_FIRST = (
    ("hp NULL", {}, {}, "hp", 3, -1),
    ("hp NULL, net GCN", {"net": 0}, {}, "hp", 3, -1),
    ("hp NULL, kNN k = 0", {"graph": 1, "k": 0}, {}, "hp", 3, -1),
)
# 2. the configuration and hp: swarm_gat3_td_grad's codes (tests/test_gat3_td_host.py)
_TD_CONFIG = (
    ("N = 0", {"N": 0}, {}, -1),
    ("N = 33", {"N": 33}, {}, -1),
    ("B = 0", {"B": 0}, {}, -1),
    ("batch = 0", {}, {"batch": 0}, -1),
    ("batch = 0, net GCN", {"net": 0}, {"batch": 0}, -1),
    ("graph 4", {"graph": 4}, {}, -1),
    ("GAT3 with GCNConv", {"conv": 1}, {}, -1),
    ("net 2", {"net": 2}, {}, -1),
    ("kNN k = 0", {"graph": 1, "k": 0}, {}, -2),
    ("kNN k = N + 1", {"graph": 1, "k": 9}, {}, -2),
    ("net GCN, kNN k = 0", {"net": 0, "graph": 1, "k": 0}, {}, -2),   # the config is checked before the net
    ("radius 0", {"graph": 3}, {}, -1),
    ("update_target_every = 0", {}, {"every": 0}, -1),
    ("update_target_every = 0, net GCN", {"net": 0}, {"every": 0}, -1),
    ("world_size = 0", {}, {"world": 0}, -1),
    ("net GCN", {"net": 0}, {}, -4),
    ("net GCN with GCNConv", {"net": 0, "conv": 1}, {}, -4),
    ("net GCN, world_size = 2", {"net": 0}, {"world": 2}, -4),
    ("net GCN, dense graph", {"net": 0, "graph": 2}, {}, -4),
    ("world_size = 2", {}, {"world": 2}, -4),
    ("world_size = 2, dense graph", {"graph": 2}, {"world": 2}, -4),
    ("dense graph", {"graph": 2}, {}, -1),
)
# 2. the configuration of the act entry: swarm_act_step's codes, then the net
_ACT_CONFIG = (
    ("N = 0", {"N": 0}, -1),
    ("N = 33", {"N": 33}, -1),
    ("B = -1", {"B": -1}, -1),
    ("graph 4", {"graph": 4}, -1),
    ("dense graph", {"graph": 2}, -1),
    ("dense graph, net GCN", {"graph": 2, "net": 0}, -1),
    ("scenario 3", {"scen": 3}, -1),
    ("Flocking with one agent", {"N": 1}, -1),
    ("conv 2", {"conv": 2}, -1),
    ("GAT3 with GCNConv", {"conv": 1}, -1),
    ("net 2", {"net": 2}, -1),
    ("kNN k = 0", {"graph": 1, "k": 0}, -2),
    ("kNN k = N + 1", {"graph": 1, "k": 9}, -2),
    ("net GCN, kNN k = 0", {"net": 0, "graph": 1, "k": 0}, -2),
    ("radius 0", {"graph": 3}, -1),
    ("net GCN", {"net": 0}, -4),
    ("net GCN with GCNConv", {"net": 0, "conv": 1}, -4),
    ("net GCN, no envs", {"net": 0, "B": 0}, -4),    # the net is refused before the empty launch returns 0
    # 3. nothing to do
    ("no envs", {"B": 0}, 0),
    ("no envs, kNN", {"B": 0, "graph": 1, "k": 8}, 0),
)


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


def _learn(fn, L, over, hp_over, null, n, table):
    cfg, hp = _cfg_hp(L, over, hp_over)
    return fn(None if null == "cfg" else ctypes.byref(cfg), None if null == "hp" else ctypes.byref(hp), table,
              None if null == "members" else 1, n, None)


def _act(lib, L, over, null, n):
    cfg, _ = _cfg_hp(L, over, {})
    return lib.swarm_pop_gat3_act_step(None if null == "cfg" else ctypes.byref(cfg), None if null == "members" else 1,
                                       n, None)


@pytest.mark.parametrize("name", ["swarm_pop_gat3_td_grad", "swarm_pop_gat3_adam_step"])
def test_learner_entry_points_error_codes_are_pinned(name):
    L, lib = _host_lib()
    fn = getattr(lib, name)
    for table in (None, 1):   # member_hp NULL (the shared hp) or a table: the same checks
        for what, over, hp_over, null, n, code in _FIRST + _HP_FIRST:
            assert _learn(fn, L, over, hp_over, null, n, table) == code, (what, table)
        for what, over, hp_over, code in _TD_CONFIG:
            for n in (1, 3, 65535):
                assert _learn(fn, L, over, hp_over, None, n, table) == code, (what, n, table)
        for over in ({"N": 32, "graph": 3, "radius": 0.5}, {"N": 17, "graph": 1, "k": 17}):
            assert _learn(fn, L, over, {}, "members", 3, table) == -1, over


def test_act_entry_point_error_codes_are_pinned():
    L, lib = _host_lib()
    for what, over, hp_over, null, n, code in _FIRST:
        assert _act(lib, L, over, null, n) == code, what
    assert _act(lib, L, {"B": 0}, "members", 3) == -1 and _act(lib, L, {"B": 0}, None, 0) == -1
    for what, over, code in _ACT_CONFIG:
        for n in (1, 3, 65535):
            assert _act(lib, L, over, None, n) == code, (what, n)


def test_act_entry_point_returns_what_swarm_act_step_returns():
    """every configuration: the lone entry point's code, but the one-layer network's"""
    L, lib = _host_lib()
    for what, over, code in _ACT_CONFIG:
        cfg, _ = _cfg_hp(L, over, {})
        if code == -4:
            continue   # swarm_act_step runs the one-layer network too
        assert lib.swarm_act_step(ctypes.byref(cfg), 1, 1, None, 1, None, None) == code, what


def test_entry_points_are_declared_everywhere():
    L, lib = _host_lib()
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("swarm_pop_gat3_act_step", "swarm_pop_gat3_td_grad", "swarm_pop_gat3_adam_step"):
        assert name in L.EXPORTED and hasattr(lib, name)
        assert f"int {name}(" in hdr
        assert f"`{name}" in doc
    assert "typedef struct swarm_gat3_member {" in hdr
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10 and "#define SWARM_ABI_VERSION 10" in hdr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_member_layout_matches_the_header(tmp_path):
    """tests/test_abi_layout.py's method on swarm_gat3_member"""
    import swarm_amd._lib as L
    cls, name = L.SwarmGat3Member, "swarm_gat3_member"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_hip.h"', "int main(void) {",
             f'  printf("{name} size %zu\\n", sizeof({name}));',
             '  printf("grad floats %d\\n", SWARM_GAT3_GRAD_FLOATS);']
    for field, _ in cls._fields_:
        lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert int(got[f"{name} size"]) == ctypes.sizeof(cls)
    for field, _ in cls._fields_:
        assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, field
    assert [f for f, _ in cls._fields_] == ["seed", "state", "replay", "params", "target", "adam_m", "adam_v", "grad",
                                            "ctrl", "out", "slabs", "sample_out"]
    assert int(got["grad floats"]) == L.GAT3_GRAD_FLOATS


def test_exported_names():
    import swarm_amd
    from swarm_amd import population
    sys.path.insert(0, os.path.join(ROOT, "compat", "src", "training"))   # as the reference's scripts import it
    try:
        compat = importlib.import_module("train_gcn_dqn")
    finally:
        sys.path.pop(0)
        sys.modules.pop("train_gcn_dqn", None)
    for name in ("SwarmGat3Population", "Gat3PopulationTrainer"):
        assert name in swarm_amd.__all__ and name in compat.__all__
        assert getattr(compat, name) is getattr(swarm_amd, name)
    assert swarm_amd.SwarmGat3Population is population.SwarmGat3Population
    # the two populations share one base and neither is the other
    assert population.SwarmPopulation.__mro__[1] is population.SwarmGat3Population.__mro__[1]
    assert swarm_amd.SwarmGat3Population.member_class is swarm_amd.SwarmGat3Engine
    assert not hasattr(swarm_amd.Gat3PopulationTrainer, "_pbt_round") and hasattr(swarm_amd.PopulationTrainer, "_pbt_round")
    for shared in ("set_member_hp", "reset", "set_eps", "capture", "read_ctrl", "evaluate"):
        assert getattr(population.SwarmGat3Population, shared) is getattr(population.SwarmPopulation, shared), shared
