"""Population training, host side (CPU only; nothing is launched): the return codes of
swarm_pop_train_tick / swarm_pop_reduce_advance before any launch, the exports, the layout of
swarm_pop_member as ctypes mirrors it, and SwarmPopulation's argument checks."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_UNSUPPORTED = -1, -4


def _host_lib():
    import swarm_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load(require_gpu=False)


def _cfg(L, **over):
    kw = dict(n_envs=1, n_agents=5, scenario=L.SWARM_GOTO, graph=L.GRAPH_COMPLETE, knn_k=5, conv=L.CONV_GAT,
              env_offset=0, flags=L.F_SHARED_RESET, seed=0, radius=0.3, net=L.NET_GCN)
    kw.update(over)
    return L.SwarmConfig(*[kw[n] for n, _ in L.SwarmConfig._fields_])


def _hp(L, **over):
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, gamma=0.99, batch=32, update_target_every=200,
              world_size=1, flags=0, lr_d=1e-3, beta1_d=0.9, beta2_d=0.999)
    kw.update(over)
    return L.SwarmAdamCfg(*[kw[n] for n, _ in L.SwarmAdamCfg._fields_])


# a descriptor table the library must never look at: every case below returns before any launch
# (the address is a host array; a launch with it would fault, and no GPU is needed to return)
def _calls(L, lib):
    table = (L.SwarmPopMember * 2)()
    members = ctypes.addressof(table)
    for name in ("swarm_pop_train_tick", "swarm_pop_reduce_advance"):
        fn = getattr(lib, name)
        yield name, table, (lambda cfg, hp, mem=members, n=2, fn=fn:
                            fn(ctypes.byref(cfg) if cfg is not None else None,
                               ctypes.byref(hp) if hp is not None else None, mem, n, None))


def test_return_codes_before_any_launch():
    L, lib = _host_lib()
    for name, _keep, call in _calls(L, lib):
        ok_cfg, ok_hp = _cfg(L), _hp(L)
        assert call(None, ok_hp) == E_BADARG, name
        assert call(ok_cfg, None) == E_BADARG, name
        assert call(ok_cfg, ok_hp, mem=None) == E_BADARG, name
        assert call(ok_cfg, ok_hp, n=0) == E_BADARG, name
        assert call(ok_cfg, ok_hp, n=-3) == E_BADARG, name
        assert call(ok_cfg, _hp(L, world_size=2)) == E_BADARG, name
        assert call(_cfg(L, n_agents=17), ok_hp) == E_UNSUPPORTED, name
        assert call(_cfg(L, net=L.NET_GAT3), ok_hp) == E_UNSUPPORTED, name
        assert call(ok_cfg, _hp(L, batch=0)) == E_BADARG, name
        assert call(ok_cfg, _hp(L, update_target_every=0)) == E_BADARG, name


def test_empty_environment_batch_is_unsupported_as_for_the_lone_tick():
    """n_envs = 0 in an otherwise valid configuration: swarm_train_tick has no kernel for it
    (swarm_train_tick_supported is 0, and the call returns SWARM_E_UNSUPPORTED); both population
    calls return the same code."""
    L, lib = _host_lib()
    cfg = _cfg(L, n_envs=0)
    assert lib.swarm_train_tick_supported(ctypes.byref(cfg)) == 0
    dummy = ctypes.c_uint64(0)   # non-null arguments of the lone tick; it returns before using them
    p = ctypes.addressof(dummy)
    lr, rep, hp = L.SwarmLearner(), L.SwarmReplay(), _hp(L)
    lone = lib.swarm_train_tick(ctypes.byref(cfg), ctypes.byref(hp), ctypes.byref(lr), p, ctypes.byref(rep), p, None,
                                p, p, None, None)
    assert lone == E_UNSUPPORTED
    for name, _keep, call in _calls(L, lib):
        assert call(cfg, hp) == lone, name


def test_symbols_are_exported_and_documented():
    L, lib = _host_lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    for name in ("swarm_pop_train_tick", "swarm_pop_reduce_advance"):
        assert hasattr(raw, name), name
        assert name in L.EXPORTED, name
        assert f"`{name}" in guide, name
        assert f"int {name}(" in hdr, name
    assert "swarm_pop_member" in guide
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10
    assert "#define SWARM_ABI_VERSION 10" in hdr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_pop_member_layout_matches_the_header(tmp_path):
    """ctypes' SwarmPopMember against a C compiler's layout of swarm_pop_member: the size, every
    field's offset, and the offsets inside the nested structs (as tests/test_abi_layout.py does
    for the other structs)."""
    import swarm_amd._lib as L
    cls = L.SwarmPopMember
    paths = []   # (C member path, ctypes offset)
    for field, typ in cls._fields_:
        base = getattr(cls, field).offset
        paths.append((field, base))
        if issubclass(typ, ctypes.Structure):
            paths += [(f"{field}.{sub}", base + getattr(typ, sub).offset) for sub, _ in typ._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(swarm_pop_member));']
    lines += [f'  printf("{p} %zu\\n", offsetof(swarm_pop_member, {p}));' for p, _ in paths]
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 232
    assert len(paths) == 9 + 6 + 8 + 10
    for p, off in paths:
        assert int(got[p]) == off, p


def test_population_refuses_what_it_cannot_tick_together():
    """Checked before any engine is built, so without a GPU."""
    from swarm_amd import SwarmPopulation
    kw = dict(scenario="GoTo", n_agents=5, n_envs=1)
    with pytest.raises(ValueError):
        SwarmPopulation(seeds=[0, 1], learn=False, **kw)
    with pytest.raises(ValueError):
        SwarmPopulation(seeds=[0, 1], world_size=2, **kw)
    with pytest.raises(ValueError):
        SwarmPopulation(seeds=[0, 1], peer=object(), **kw)
    with pytest.raises(ValueError):
        SwarmPopulation(seeds=[], **kw)
    with pytest.raises(ValueError):
        SwarmPopulation(seeds=[0], seed=3, **kw)
