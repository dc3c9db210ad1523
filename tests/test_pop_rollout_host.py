"""Population rollouts, host side (CPU only; nothing is launched): the return codes of
swarm_pop_rollout before any launch, held against swarm_rollout's own over a grid of
configurations, the export, and the layout of swarm_pop_actor as ctypes mirrors it."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

from tests.test_population_host import _cfg, _host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_KNN_K = -1, -2


# a descriptor table the library must never look at: every case below returns before any launch
# (the address is a host array; a launch with it would fault, and no GPU is needed to return)
def _pop_call(L, lib):
    table = (L.SwarmPopActor * 2)()
    actors = ctypes.addressof(table)

    def call(cfg, mem=actors, n=2, n_ticks=5):
        return lib.swarm_pop_rollout(ctypes.byref(cfg) if cfg is not None else None, mem, n, n_ticks, None)
    return table, call


def _lone_call(L, lib):
    dummy = (ctypes.c_float * 4)()   # non-null params / state; swarm_rollout returns before using them
    p = ctypes.addressof(dummy)

    def call(cfg, n_ticks=5):
        return lib.swarm_rollout(ctypes.byref(cfg), p, p, n_ticks, 0, 0.0, None, None)
    return dummy, call


def test_return_codes_in_their_order():
    L, lib = _host_lib()
    _keep, call = _pop_call(L, lib)
    ok = _cfg(L, graph=L.GRAPH_KNN, knn_k=5)
    bad_k = _cfg(L, graph=L.GRAPH_KNN, knn_k=6)
    # 1. NULL cfg or actors, n_actors outside 1..65535: before anything of the configuration
    assert call(None) == E_BADARG
    for cfg in (ok, bad_k):
        assert call(cfg, mem=None) == E_BADARG
        for n in (0, -3, 65536, 1 << 30):
            assert call(cfg, n=n) == E_BADARG, n
    # 2. then the configuration, ahead of n_ticks
    assert call(bad_k) == E_KNN_K
    assert call(bad_k, n_ticks=-1) == E_KNN_K
    assert call(bad_k, n_ticks=0) == E_KNN_K
    assert call(bad_k, n=65535) == E_KNN_K
    # 3. then a negative n_ticks, also with no environments
    assert call(ok, n_ticks=-1) == E_BADARG
    assert call(_cfg(L, n_envs=0), n_ticks=-1) == E_BADARG
    # 4. nothing to do: 0, and the table is never read (it is host memory)
    assert call(ok, n_ticks=0) == 0
    assert call(ok, n_ticks=0, n=65535) == 0
    assert call(_cfg(L, n_envs=0)) == 0
    assert call(_cfg(L, n_envs=0), n_ticks=0) == 0


def test_every_configuration_returns_what_swarm_rollout_returns():
    """Over the grid, with n_ticks = 0 (or no environments) wherever the configuration is valid,
    so that neither call launches; -1 ticks as well, which both refuse after the configuration."""
    L, lib = _host_lib()
    _keep_a, pop = _pop_call(L, lib)
    _keep_b, lone = _lone_call(L, lib)
    graphs = [dict(graph=L.GRAPH_COMPLETE), dict(graph=L.GRAPH_KNN, knn_k=1), dict(graph=L.GRAPH_KNN, knn_k=5),
              dict(graph=L.GRAPH_KNN, knn_k=33), dict(graph=L.GRAPH_KNN, knn_k=0), dict(graph=L.GRAPH_DENSE),
              dict(graph=L.GRAPH_RADIUS, radius=0.3), dict(graph=L.GRAPH_RADIUS, radius=0.0),
              dict(graph=L.GRAPH_RADIUS, radius=-1.0), dict(graph=7)]
    nets = [dict(net=L.NET_GCN, conv=L.CONV_GAT), dict(net=L.NET_GCN, conv=L.CONV_GCN),
            dict(net=L.NET_GAT3, conv=L.CONV_GAT), dict(net=L.NET_GAT3, conv=L.CONV_GCN), dict(net=5), dict(conv=3)]
    scens = (L.SWARM_GOTO, L.SWARM_OBSTACLE_AVOIDANCE, L.SWARM_FLOCKING, 9)
    seen = set()
    for n_agents, g, nt, scen, n_envs in itertools.product((0, 1, 32, 33, 5), graphs, nets, scens, (0, 1, 6, -1)):
        cfg = _cfg(L, n_agents=n_agents, scenario=scen, n_envs=n_envs, **g, **nt)
        for n_ticks in (0, -1):
            want = lone(cfg, n_ticks)
            assert pop(cfg, n_ticks=n_ticks) == want, (n_agents, g, nt, scen, n_envs, n_ticks)
            seen.add(want)
        if n_envs == 0 and lone(cfg, 0) == 0:   # no environments: a positive n_ticks launches nothing either
            assert pop(cfg, n_ticks=5) == lone(cfg, 5) == 0
    assert seen == {0, E_BADARG, E_KNN_K}
    # the grid's named corners, as swarm_rollout answers them
    assert pop(_cfg(L, n_agents=0), n_ticks=0) == E_BADARG
    assert pop(_cfg(L, n_agents=33), n_ticks=0) == E_BADARG
    assert pop(_cfg(L, n_agents=32, graph=L.GRAPH_KNN, knn_k=32), n_ticks=0) == 0
    assert pop(_cfg(L, n_agents=1, graph=L.GRAPH_KNN, knn_k=2), n_ticks=0) == E_KNN_K
    assert pop(_cfg(L, graph=L.GRAPH_DENSE), n_ticks=0) == E_BADARG
    assert pop(_cfg(L, graph=L.GRAPH_RADIUS, radius=0.0), n_ticks=0) == E_BADARG
    assert pop(_cfg(L, net=L.NET_GAT3, conv=L.CONV_GCN), n_ticks=0) == E_BADARG
    assert pop(_cfg(L, net=L.NET_GAT3, conv=L.CONV_GAT), n_ticks=0) == 0
    assert pop(_cfg(L, scenario=L.SWARM_FLOCKING, n_agents=1), n_ticks=0) == E_BADARG


def test_symbol_is_exported_and_documented():
    L, lib = _host_lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    assert hasattr(raw, "swarm_pop_rollout")
    assert "swarm_pop_rollout" in L.EXPORTED
    assert "`swarm_pop_rollout`" in guide and "swarm_pop_actor" in guide
    assert "int swarm_pop_rollout(" in hdr and "} swarm_pop_actor;" in hdr
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10
    assert "#define SWARM_ABI_VERSION 10" in hdr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_pop_actor_layout_matches_the_header(tmp_path):
    """ctypes' SwarmPopActor against a C compiler's layout of swarm_pop_actor: the size, every
    field's offset and the offsets inside the nested swarm_act_out (as
    test_pop_member_layout_matches_the_header does for swarm_pop_member)."""
    import swarm_amd._lib as L
    cls = L.SwarmPopActor
    paths = []   # (C member path, ctypes offset)
    for field, typ in cls._fields_:
        base = getattr(cls, field).offset
        paths.append((field, base))
        if issubclass(typ, ctypes.Structure):
            paths += [(f"{field}.{sub}", base + getattr(typ, sub).offset) for sub, _ in typ._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(swarm_pop_actor));']
    lines += [f'  printf("{p} %zu\\n", offsetof(swarm_pop_actor, {p}));' for p, _ in paths]
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 112
    assert [p for p, _ in paths if "." not in p] == ["seed", "params", "state", "out", "tick0", "eps"]
    assert len(paths) == 6 + 10
    for p, off in paths:
        assert int(got[p]) == off, p
