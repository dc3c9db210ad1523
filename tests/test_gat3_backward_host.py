"""CPU-only tests of swarm_gat3_q_backward's host side (what it returns before it would launch
anything), its declarations, the slab bound of its workspace and the ``GAT3`` class's keywords.
No GPU compute is called here."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (what, config overrides, NULL argument or None, expected code), in the entry point's order of
# checks: every call is rejected, so 1 can stand in for every device pointer.  Base config: 8 agents,
# 4 graphs, GoTo, complete graph, GAT, the three-layer net.
_BASE = dict(B=4, N=8, scen=0, graph=0, k=0, conv=0, radius=0.0, net=1)
_REJECTED = (
    ("cfg NULL", {}, "cfg", -1),
    ("N = 0", {"N": 0}, None, -1),
    ("N = 33", {"N": 33}, None, -1),
    ("B = 0", {"B": 0}, None, -1),
    ("B = -1", {"B": -1}, None, -1),
    ("scenario 3", {"scen": 3}, None, -1),
    ("graph 4", {"graph": 4}, None, -1),
    ("conv 2", {"conv": 2}, None, -1),
    ("net GCN", {"net": 0}, None, -4),
    ("net GCN with GCNConv", {"net": 0, "conv": 1}, None, -4),
    ("net GCN, params NULL", {"net": 0}, "params", -4),        # the net is checked before the pointers
    ("GAT3 with GCNConv", {"conv": 1}, None, -1),
    ("kNN k = 0", {"graph": 1, "k": 0}, None, -2),
    ("kNN k = N + 1", {"graph": 1, "k": 9}, None, -2),
    ("net GCN, kNN k = 0", {"net": 0, "graph": 1, "k": 0}, None, -2),   # the config is checked before the net
    ("radius 0", {"graph": 3, "radius": 0.0}, None, -1),
    ("radius < 0", {"graph": 3, "radius": -1.0}, None, -1),
    ("dense, mult NULL", {"graph": 2}, "mult", -1),
    ("params NULL", {}, "params", -1),
    ("x NULL", {}, "x", -1),
    ("dq NULL", {}, "dq", -1),
    ("workspace NULL", {}, "workspace", -1),
    ("grad NULL", {}, "grad", -1),
    ("dense, params NULL", {"graph": 2}, "params", -1),
    ("N = 32, radius, x NULL", {"N": 32, "graph": 3, "radius": 0.5}, "x", -1),
)


def _host_lib():
    import swarm_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load(require_gpu=False)


def test_gat3_q_backward_error_codes_are_pinned():
    L, lib = _host_lib()
    for what, over, null, code in _REJECTED:
        c = dict(_BASE, **over)
        cfg = L.SwarmConfig(c["B"], c["N"], c["scen"], c["graph"], c["k"], c["conv"], 0, 0, 7, c["radius"], c["net"])
        P = {n: (None if n == null else 1) for n in ("params", "x", "mult", "dq", "workspace", "grad")}
        if c["graph"] != 2 and null != "mult":
            P["mult"] = None   # mult is NULL unless the graph is dense
        got = lib.swarm_gat3_q_backward(None if null == "cfg" else ctypes.byref(cfg), P["params"], P["x"], P["mult"],
                                        P["dq"], P["workspace"], P["grad"], None)
        assert got == code, (what, got)


def test_closed_doors_stay_closed():
    """swarm_q_backward still refuses the three-layer net: the feature is a new entry point."""
    L, lib = _host_lib()
    cfg = L.SwarmConfig(4, 8, 0, 0, 0, 0, 0, 0, 7, 0.0, L.NET_GAT3)
    assert lib.swarm_q_backward(ctypes.byref(cfg), 1, 1, None, 1, 1, 1, None) == -4


def test_gat3_q_backward_is_declared_everywhere():
    L, lib = _host_lib()
    assert "swarm_gat3_q_backward" in L.EXPORTED and hasattr(lib, "swarm_gat3_q_backward")
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    assert "int swarm_gat3_q_backward(" in hdr
    assert "#define SWARM_GAT3_GRAD_FLOATS 416" in hdr and L.GAT3_GRAD_FLOATS == 416
    assert "`swarm_gat3_q_backward" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10


def test_slabs_fit_the_td_workspace():
    """The backward kernel writes one 416-float slab per block of graphs into the workspace the
    caller sized with swarm_td_workspace_floats(cfg, n_envs)."""
    from swarm_amd.graph import gat3_backward_slab_floats
    L, lib = _host_lib()
    for N in (8, 16, 32, 1, 9, 17):
        for B in (1, 8, 33):
            cfg = L.SwarmConfig(B, N, 0, 0, 0, 0, 0, 0, 0, 0.0, L.NET_GAT3)
            have = lib.swarm_td_workspace_floats(ctypes.byref(cfg), B)
            need = gat3_backward_slab_floats(N, B)
            assert need >= 416 and need % 416 == 0
            assert have >= need, (N, B, have, need)
    assert gat3_backward_slab_floats(8, 33) == 9 * 416 and gat3_backward_slab_floats(17, 33) == 17 * 416


def test_gat3_class_keywords():
    import importlib
    import sys
    import swarm_amd
    sys.path.insert(0, os.path.join(ROOT, "compat", "src", "training"))   # as the reference's scripts import it
    try:
        compat = importlib.import_module("train_gcn_dqn")
    finally:
        sys.path.pop(0)
        sys.modules.pop("train_gcn_dqn", None)
    assert compat.GAT3 is swarm_amd.GAT3 and "GAT3" in swarm_amd.__all__ and "GAT3" in compat.__all__
    m = swarm_amd.GAT3()
    assert isinstance(m, swarm_amd.GCN) and m.autograd is False and m.layers == 3 and m.net == "gat3"
    assert swarm_amd.GAT3(autograd=True).autograd is True
    with pytest.raises(ValueError, match="GAT3"):
        swarm_amd.GCN(7, 8, 9, layers=3, autograd=True)
    with pytest.raises(ValueError):
        swarm_amd.GAT3(conv="gcn")
    assert list(m.state_dict()) == list(swarm_amd.GCN(7, 8, 9, layers=3).state_dict())
    sd = m.state_dict()
    a = swarm_amd.GCN.from_state_dict(sd)
    b = swarm_amd.GCN.from_state_dict(sd, "gat", autograd=True)
    assert isinstance(a, swarm_amd.GAT3) and a.autograd is False
    assert isinstance(b, swarm_amd.GAT3) and b.autograd is True and b.layers == 3 and b.net == "gat3"
    assert list(b.state_dict()) == list(sd)
    one = swarm_amd.GCN.from_state_dict(swarm_amd.GCN(7, 32, 9).state_dict(), autograd=True)
    assert not isinstance(one, swarm_amd.GAT3) and one.autograd is True
