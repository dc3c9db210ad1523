"""Per-member optimizer hyper-parameters of a population, host side (CPU only; nothing is
launched): the exports and the return codes of swarm_pop_train_tick_hp /
swarm_pop_reduce_advance_hp before any launch, and SwarmPopulation's parsing of its per-member
keyword arguments (checked before any engine is built)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("swarm_pop_train_tick_hp", "swarm_pop_reduce_advance_hp")


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


def test_symbols_are_exported_and_documented():
    L, lib = _host_lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.EXPORTED, name
        assert f"`{name}" in guide, name
        assert f"int {name}(" in hdr, name
    # additions only: the version stays
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10


# (what is wrong, cfg overrides, shared-hp overrides, call overrides) -> status.  1 stands for a
# device pointer: every case returns before any launch, so nothing ever follows it.
E_BADARG, E_UNSUPPORTED = -1, -4
RETURN_CODES = (
    ("NULL cfg", None, {}, {}, -1),
    ("NULL hp", {}, None, {}, -1),
    ("NULL member_hp", {}, {}, dict(member_hp=None), -1),
    ("NULL members", {}, {}, dict(members=None), -1),
    ("no members", {}, {}, dict(n=0), -1),
    ("65536 members", {}, {}, dict(n=65536), -1),
    ("world_size 2", {}, dict(world_size=2), {}, -1),
    ("17 agents", dict(n_agents=17), {}, {}, -4),
    ("the GAT3 net", "gat3", {}, {}, -4),
    ("batch 0", {}, dict(batch=0), {}, -1),
)


@pytest.mark.parametrize("name", NAMES)
def test_return_codes_before_any_launch(name):
    L, lib = _host_lib()
    fn = getattr(lib, name)
    for what, cfg_over, hp_over, call_over, status in RETURN_CODES:
        if cfg_over == "gat3":
            cfg_over = dict(net=L.NET_GAT3)
        cfg = None if cfg_over is None else _cfg(L, **cfg_over)
        hp = None if hp_over is None else _hp(L, **hp_over)
        args = dict(member_hp=1, members=1, n=2)
        args.update(call_over)
        got = fn(ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(hp) if hp is not None else None,
                 args["member_hp"], args["members"], args["n"], None)
        assert got == status, f"{name}: {what}"


def test_checks_come_in_the_shared_pairs_order():
    """Two faults at once return the code of the one the shared pair checks first: world_size
    before the configuration, the configuration before batch."""
    L, lib = _host_lib()
    for name in NAMES:
        fn = getattr(lib, name)
        old = getattr(lib, name[:-3])
        for cfg, hp in ((_cfg(L, n_agents=17), _hp(L, world_size=2)), (_cfg(L, n_agents=17), _hp(L, batch=0))):
            want = old(ctypes.byref(cfg), ctypes.byref(hp), 1, 2, None)
            assert fn(ctypes.byref(cfg), ctypes.byref(hp), 1, 1, 2, None) == want, name
        assert want == E_UNSUPPORTED


def test_member_keyword_parsing_needs_no_gpu():
    from swarm_amd.population import member_hp_kwargs
    base = dict(scenario="GoTo", n_agents=5, n_envs=1)
    # scalars as before: every member gets the same keyword arguments
    assert member_hp_kwargs(2, dict(base, lr=1e-3)) == [dict(base, lr=1e-3)] * 2
    # a bare pair of floats is the shared betas, also when there are two members
    got = member_hp_kwargs(2, dict(base, betas=(0.9, 0.999)))
    assert [kw["betas"] for kw in got] == [(0.9, 0.999), (0.9, 0.999)]
    got = member_hp_kwargs(2, dict(base, betas=[(0.9, 0.999), (0.8, 0.99)], lr=[1e-3, 3e-4], gamma=0.9))
    assert [kw["betas"] for kw in got] == [(0.9, 0.999), (0.8, 0.99)]
    assert [kw["lr"] for kw in got] == [1e-3, 3e-4] and [kw["gamma"] for kw in got] == [0.9, 0.9]
    assert all(kw["scenario"] == "GoTo" for kw in got)
    got = member_hp_kwargs(3, dict(base, update_target_every=(2, 3, 5), adam_eps=[1e-8, 1e-3, 1e-5], max_norm=0.5))
    assert [kw["update_target_every"] for kw in got] == [2, 3, 5]
    assert [kw["adam_eps"] for kw in got] == [1e-8, 1e-3, 1e-5] and [kw["max_norm"] for kw in got] == [0.5] * 3


@pytest.mark.parametrize("bad", [
    dict(lr=[1e-3, 1e-4, 1e-5]),                      # three values for two members
    dict(gamma=[0.9]),
    dict(betas=[(0.9, 0.999)]),
    dict(betas=[(0.9, 0.999), (0.9, 0.999), (0.9, 0.999)]),
    dict(update_target_every=[3, 0]),                 # the kernels take a tick count modulo it
    dict(update_target_every=0),
    dict(lr=[1e-3, float("nan")]),
    dict(adam_eps=[1e-8, float("inf")]),
    dict(betas=[(0.9, 0.999), (0.9, 1.0)]),
])
def test_population_refuses_bad_member_values_before_building_an_engine(bad):
    """SwarmPopulation raises from its argument parsing: no engine, so no GPU, is involved."""
    from swarm_amd import SwarmPopulation
    from swarm_amd.population import member_hp_kwargs
    kw = dict(scenario="GoTo", n_agents=5, n_envs=1)
    with pytest.raises(ValueError):
        member_hp_kwargs(2, dict(kw, **bad))
    with pytest.raises(ValueError):
        SwarmPopulation(seeds=[0, 1], **kw, **bad)


def test_set_hp_value_checks():
    from swarm_amd.engine import HP_FIELDS, check_hp_values
    assert set(HP_FIELDS) == {"lr", "gamma", "betas", "adam_eps", "max_norm", "update_target_every"}
    check_hp_values(lr=1e-3, gamma=0.99, betas=(0.9, 0.999), adam_eps=1e-8, max_norm=1.0, update_target_every=1)
    for bad in (dict(batch=4), dict(lr=-1.0), dict(update_target_every=2.5), dict(betas=0.9), dict(max_norm=float("nan"))):
        with pytest.raises(ValueError):
            check_hp_values(**bad)
