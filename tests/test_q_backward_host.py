"""CPU-only tests of swarm_q_backward's host side (what it returns before it would launch
anything) and of the ``autograd`` keyword of ``GCN``.  No GPU compute is called here."""
import ctypes
import os

import pytest

# (what, config overrides, NULL argument or None, expected code): every call is rejected, so 1 can
# stand in for every device pointer.  Base config: 8 agents, 4 graphs, GoTo, complete graph, GAT, GCN net.
_BASE = dict(B=4, N=8, scen=0, graph=0, k=0, conv=0, radius=0.0, net=0)
_REJECTED = (
    ("cfg NULL", {}, "cfg", -1),
    ("N = 0", {"N": 0}, None, -1),
    ("N = 33", {"N": 33}, None, -1),
    ("B = 0", {"B": 0}, None, -1),
    ("B = -1", {"B": -1}, None, -1),
    ("scenario 3", {"scen": 3}, None, -1),
    ("flocking with one agent", {"scen": 2, "N": 1}, None, -1),
    ("graph 4", {"graph": 4}, None, -1),
    ("graph -1", {"graph": -1}, None, -1),
    ("conv 2", {"conv": 2}, None, -1),
    ("net GAT3", {"net": 1}, None, -4),
    ("net GAT3 with GCNConv", {"net": 1, "conv": 1}, None, -4),
    ("kNN k = 0", {"graph": 1, "k": 0}, None, -2),
    ("kNN k = N + 1", {"graph": 1, "k": 9}, None, -2),
    ("radius 0", {"graph": 3, "radius": 0.0}, None, -1),
    ("radius < 0", {"graph": 3, "radius": -1.0}, None, -1),
    ("dense, mult NULL", {"graph": 2}, "mult", -1),
    ("params NULL", {}, "params", -1),
    ("x NULL", {}, "x", -1),
    ("dq NULL", {}, "dq", -1),
    ("workspace NULL", {}, "workspace", -1),
    ("grad NULL", {}, "grad", -1),
    ("dense, params NULL", {"graph": 2}, "params", -1),
    ("kNN, grad NULL", {"graph": 1, "k": 3}, "grad", -1),
    ("N = 32, radius, x NULL", {"N": 32, "graph": 3, "radius": 0.5}, "x", -1),
)


def _host_lib():
    import swarm_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load(require_gpu=False)


def test_q_backward_error_codes_are_pinned():
    L, lib = _host_lib()
    for what, over, null, code in _REJECTED:
        c = dict(_BASE, **over)
        cfg = L.SwarmConfig(c["B"], c["N"], c["scen"], c["graph"], c["k"], c["conv"], 0, 0, 7, c["radius"], c["net"])
        P = {n: (None if n == null else 1) for n in ("params", "x", "mult", "dq", "workspace", "grad")}
        if c["graph"] != 2 and null != "mult":
            P["mult"] = None   # mult is NULL unless the graph is dense
        got = lib.swarm_q_backward(None if null == "cfg" else ctypes.byref(cfg), P["params"], P["x"], P["mult"],
                                   P["dq"], P["workspace"], P["grad"], None)
        assert got == code, (what, got)


def test_q_backward_is_declared_everywhere():
    L, lib = _host_lib()
    assert "swarm_q_backward" in L.EXPORTED and hasattr(lib, "swarm_q_backward")
    assert lib.swarm_abi_version() == 10


def test_gcn_autograd_keyword():
    import swarm_amd
    with pytest.raises(ValueError):
        swarm_amd.GCN(7, 8, 9, layers=3, autograd=True)
    assert swarm_amd.GCN(7, 32, 9).autograd is False
    assert swarm_amd.GCN(7, 32, 9, autograd=True).autograd is True
    sd = swarm_amd.GCN(7, 32, 9).state_dict()
    assert swarm_amd.GCN.from_state_dict(sd).autograd is False
    assert swarm_amd.GCN.from_state_dict(sd, "gat", autograd=True).autograd is True
