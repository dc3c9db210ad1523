"""Population-based training, host side (CPU only; nothing is launched): the return codes of
swarm_pop_exploit before any launch and their order, the export and its documentation, the layout
of swarm_pbt_cfg as ctypes mirrors it, and the argument checks of SwarmPopulation.exploit
(population.pbt_round_cfg) and of the trainer's pbt_every (dqn.pbt_schedule)."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest

from tests.test_population_host import _host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_UNSUPPORTED = -1, -4


def _pbt(L, **over):
    kw = dict(seed=7, round=0, n_replace=1, fields=L.PBT_F_LR, perturb_lo=0.8, perturb_hi=1.2, gamma_min=0.0,
              gamma_max=0.9999, lr_min=1e-6, lr_max=1e-1)
    kw.update(over)
    return L.SwarmPbtCfg(*[kw[n] for n, _ in L.SwarmPbtCfg._fields_])


# tables the library must never look at: every case below returns before any launch (the addresses
# are host arrays; a launch with them would fault, and no GPU is needed to return)
def _call(L, lib):
    keep = ((ctypes.c_float * 8)(), (L.SwarmAdamCfg * 8)(), (L.SwarmPopMember * 8)(), (ctypes.c_int32 * 8)())
    score, hp, members, parent = (ctypes.addressof(a) for a in keep)

    def call(pbt, n=4, score=score, hp=hp, members=members, parent=parent):
        return lib.swarm_pop_exploit(ctypes.byref(pbt) if pbt is not None else None, score, hp, members, n, parent, None)
    return keep, call


def test_return_codes_in_their_order():
    L, lib = _host_lib()
    _keep, call = _call(L, lib)
    ok = _pbt(L)
    inf, nan = math.inf, math.nan
    bad_replace, bad_fields, bad_factor = _pbt(L, n_replace=3), _pbt(L, fields=4), _pbt(L, perturb_lo=0.0)
    # 1. a NULL argument, ahead of everything
    assert call(None) == E_BADARG
    for name in ("score", "hp", "members", "parent"):
        for pbt, n in ((ok, 4), (ok, 0), (ok, 5000), (bad_replace, 4)):
            assert call(pbt, n=n, **{name: None}) == E_BADARG, name
    # 2. n_members < 1, ahead of n_replace (3 of 0 members would be refused anyway: same code)
    for n in (0, -1, -(1 << 31)):
        assert call(ok, n=n) == E_BADARG, n
    # 3. too many members: UNSUPPORTED, ahead of n_replace, the fields and the factors
    for pbt in (ok, _pbt(L, n_replace=-1), _pbt(L, n_replace=4000), bad_fields, bad_factor):
        assert call(pbt, n=L.PBT_MAX_MEMBERS + 1) == E_UNSUPPORTED
        assert call(pbt, n=1 << 30) == E_UNSUPPORTED
    # 4. n_replace outside [0, n_members / 2]
    assert call(_pbt(L, n_replace=-1)) == E_BADARG
    assert call(_pbt(L, n_replace=3), n=4) == E_BADARG
    assert call(_pbt(L, n_replace=3), n=5) == E_BADARG
    assert call(_pbt(L, n_replace=1), n=1) == E_BADARG
    assert call(_pbt(L, n_replace=513), n=L.PBT_MAX_MEMBERS) == E_BADARG
    # 5. unknown fields bits
    for f in (4, 8, 7, -1, 1 << 30):
        assert call(_pbt(L, fields=f)) == E_BADARG, f
    # 6. factors and bounds: non-finite, non-positive, in the wrong order
    for over in (dict(perturb_lo=0.0), dict(perturb_lo=-0.5), dict(perturb_lo=nan), dict(perturb_hi=inf),
                 dict(perturb_hi=nan), dict(perturb_lo=1.2, perturb_hi=0.8),
                 dict(gamma_min=nan), dict(gamma_max=inf), dict(gamma_min=-inf), dict(gamma_min=0.9, gamma_max=0.5),
                 dict(lr_min=0.0), dict(lr_min=-1e-3), dict(lr_min=nan), dict(lr_max=inf), dict(lr_max=nan),
                 dict(lr_min=1e-2, lr_max=1e-3)):
        for fields in (0, L.PBT_F_LR, L.PBT_F_GAMMA, L.PBT_F_LR | L.PBT_F_GAMMA):   # checked whatever is perturbed
            assert call(_pbt(L, fields=fields, **over)) == E_BADARG, over
    # the order among 4, 5 and 6 cannot show in the code (all SWARM_E_BADARG); that 3 precedes them can, above


def test_symbol_is_exported_and_documented():
    L, lib = _host_lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "swarm_hip.h")).read()
    assert hasattr(raw, "swarm_pop_exploit")
    assert "swarm_pop_exploit" in L.EXPORTED
    assert "`swarm_pop_exploit`" in guide and "swarm_pbt_cfg" in guide
    assert "int swarm_pop_exploit(" in hdr and "} swarm_pbt_cfg;" in hdr
    for define in ("#define SWARM_PBT_F_LR 1", "#define SWARM_PBT_F_GAMMA 2", "#define SWARM_PBT_MAX_MEMBERS 1024"):
        assert define in hdr, define
    assert (L.PBT_F_LR, L.PBT_F_GAMMA, L.PBT_MAX_MEMBERS, L.STREAM_PBT) == (1, 2, 1024, 5)
    assert lib.swarm_abi_version() == L.ABI_VERSION == 10   # additive: the version stays
    assert "#define SWARM_ABI_VERSION 10" in hdr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_pbt_cfg_layout_matches_the_header(tmp_path):
    """ctypes' SwarmPbtCfg against a C compiler's layout of swarm_pbt_cfg: the size and every
    field's offset (as test_pop_member_layout_matches_the_header does for swarm_pop_member)."""
    import swarm_amd._lib as L
    cls = L.SwarmPbtCfg
    names = [f for f, _ in cls._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(swarm_pbt_cfg));']
    lines += [f'  printf("{p} %zu\\n", offsetof(swarm_pbt_cfg, {p}));' for p in names]
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 56
    assert names == ["seed", "round", "n_replace", "fields", "perturb_lo", "perturb_hi", "gamma_min", "gamma_max",
                     "lr_min", "lr_max"]
    for p in names:
        assert int(got[p]) == getattr(cls, p).offset, p


def test_exploit_argument_checks():
    """SwarmPopulation.exploit hands its arguments to population.pbt_round_cfg before it launches
    anything; the function needs no GPU (the score here is a host tensor and the device is "cpu")."""
    import torch

    import swarm_amd._lib as L
    from swarm_amd.population import pbt_round_cfg
    P = 8
    score = torch.zeros(P)

    def cfg(score=score, P=P, device="cpu", **kw):
        kw.setdefault("round", 0)
        return pbt_round_cfg(P, score, device, **kw)

    c = cfg(round=3, seed=(5 << 32) | 9, frac=0.25, fields=("lr", "gamma"), perturb=(0.5, 2.0), lr_bounds=(1e-5, 1e-2),
            gamma_bounds=(0.1, 0.99))
    assert (c.seed, c.round, c.n_replace, c.fields) == ((5 << 32) | 9, 3, 2, L.PBT_F_LR | L.PBT_F_GAMMA)
    assert (c.perturb_lo, c.perturb_hi, c.lr_min, c.lr_max) == (0.5, 2.0, 1e-5, 1e-2)
    assert cfg().n_replace == 2 and cfg().fields == L.PBT_F_LR   # the defaults: a quarter, lr only
    assert cfg(frac=0.5).n_replace == 4 and cfg(frac=0.0).n_replace == 0 and cfg(frac=0.49).n_replace == 3
    assert cfg(fields="gamma").fields == L.PBT_F_GAMMA and cfg(fields=()).fields == 0
    assert cfg(score=torch.zeros(1), P=1).n_replace == 0
    bad = [dict(frac=0.51), dict(frac=-0.1), dict(frac=math.nan), dict(frac="half"),
           dict(score=torch.zeros(P + 1)), dict(score=torch.zeros(P, 1)), dict(score=torch.zeros(P, dtype=torch.float64)),
           dict(score=[0.0] * P), dict(score=torch.zeros(2 * P)[::2]), dict(device="cuda:0"),
           dict(fields=("lr", "beta1")), dict(fields="eps"),
           dict(round=-1), dict(round=1 << 32), dict(round=1.5), dict(seed=0.5),
           dict(perturb=(0.0, 1.2)), dict(perturb=(1.2, 0.8)), dict(perturb=(0.8, math.inf)), dict(perturb=0.8),
           dict(perturb=(1e-60, 1.2)), dict(perturb=(0.8, 1e60)),
           dict(lr_bounds=(0.0, 0.1)), dict(lr_bounds=(0.1, 0.01)), dict(lr_bounds=(1e-6, math.nan)),
           dict(gamma_bounds=(0.9, 0.5)), dict(gamma_bounds=(0.0, math.inf)), dict(gamma_bounds=(0.0,)),
           dict(P=L.PBT_MAX_MEMBERS + 1, score=torch.zeros(L.PBT_MAX_MEMBERS + 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            cfg(**kw)


def test_pbt_every_must_be_a_multiple_of_eval_every():
    from swarm_amd.dqn import pbt_schedule
    assert pbt_schedule({}) is None and pbt_schedule({"eval_every": 2}) is None
    assert pbt_schedule({"eval_every": 2, "pbt_every": 2}) == 2
    assert pbt_schedule({"eval_every": 2, "pbt_every": 6}) == 6
    assert pbt_schedule({"eval_every": 1, "pbt_every": 5}) == 5
    for config in ({"pbt_every": 2}, {"eval_every": 2, "pbt_every": 3}, {"eval_every": 4, "pbt_every": 2},
                   {"eval_every": 2, "pbt_every": 0}, {"eval_every": 2, "pbt_every": -2},
                   {"eval_every": 2, "pbt_every": 2.5}, {"eval_every": 1, "pbt_every": True},
                   {"eval_every": None, "pbt_every": 2}):
        with pytest.raises(ValueError):
            pbt_schedule(config)
