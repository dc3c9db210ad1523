"""The references of tests/test_gpu_hp_reference.py, checked on the CPU for every hyper-parameter
case (tests/hp_cases.py): the float64 restatements agree with torch.optim.Adam + clip_grad_norm_
(oracle.clip_adam) within the bounds the GPU is held to, every case's sensitivity guard holds (the
reference at the case's value and at the default differ by more than 10x the asserted bound on
more than 1 % of the elements of the quantity the field acts on, so a kernel that ignores the
field cannot pass), and the fp32 restatement's rounding noise, from which the bounds are formed,
is recorded.  The state walks N_STEPS steps of torch's own optimizer from the golden weights."""
import pytest
import torch

from oracle import swarm_oracle as O
from tests import hp_cases as H
from tests.conftest import error_stats, record
from tests.test_gpu_parity_large import _clip_adam64


def _field_targets(field, value):
    """The quantities a field acts on directly (the ones its guard looks at)."""
    if field == "betas":
        return tuple(q for q, b, d in (("m", value[0], 0.9), ("v", value[1], 0.999)) if b != d)
    return {"lr": ("p",), "adam_eps": ("p",), "max_norm": ("m", "v"), "world_size": ("m", "v")}[field]


def walk(name, p_init):
    """The case's N_STEPS steps by torch from p_init: per step the inputs, torch's fp32 result, the
    float64 step, the fp32 restatement's ulp errors, the scales and max_norm."""
    hp = H.case_hp(name)
    lr, (b1, b2), eps, W = hp["lr"], hp["betas"], hp["adam_eps"], hp["world_size"]
    p, m, v, out = p_init.clone(), None, None, []
    for s in range(H.N_STEPS):
        g = H.synthetic_grad(name, s)
        mn = H.step_max_norm(name, s, g, W)
        sc = H.adam_scalars(lr, b1, b2, s)
        r64 = H.adam_ref64(p, g, m, v, sc, eps, mn, W)
        sc_ = H.scales(p, m, v, r64, sc, lr)
        noise = H.ulp_errors(H.adam_np32(p, g, m, v, sc, eps, mn, W), r64, sc_)
        g_w = g if W == 1 else g * torch.tensor(1.0 / W, dtype=torch.float32)
        zero = torch.zeros_like(p)
        tp, tm, tv, tn = O.clip_adam(p, g_w, zero if m is None else m, zero if v is None else v, s, lr=lr,
                                     betas=(b1, b2), eps=eps, max_norm=mn)
        out.append(dict(p0=p, m0=m, v0=v, g=g, max_norm=mn, sc=sc, r64=r64, scales=sc_, noise=noise,
                        torch=dict(p=tp, m=tm, v=tv, norm=tn)))
        p, m, v = tp, tm, tv
    return hp, out


@pytest.fixture(scope="module")
def p_init(golden_weights):
    return torch.tensor(golden_weights["go_to"][0])


@pytest.mark.parametrize("name", list(H.CASES))
def test_float64_restatement_agrees_with_torch_and_guard_holds(p_init, name):
    hp, steps = walk(name, p_init)
    noise = {k: max(st["noise"][k] for st in steps) for k in H.PROJECT_ULP}
    bound = H.bounds_from_noise(noise)
    record(f"hp {name}: fp32 restatement vs float64, largest over {H.N_STEPS} steps (ulp)", noise)
    record(f"hp {name}: asserted bounds (ulp)", bound)
    lr, (b1, b2), eps, W = hp["lr"], hp["betas"], hp["adam_eps"], hp["world_size"]
    worst = dict.fromkeys(H.PROJECT_ULP, 0.0)
    for s, st in enumerate(steps):
        # torch's fp32 step against the float64 restatement from the fp32 inputs
        err = H.ulp_errors(st["torch"], st["r64"], st["scales"])
        worst = {k: max(worst[k], err[k]) for k in worst}
        for k in err:
            assert err[k] <= bound[k], (name, s, k, err[k], bound[k])
        # and against _clip_adam64 (Python-float hyper-parameters), on the weights and the norm
        p64, m64, v64, n64 = _clip_adam64(st["p0"], st["g"], st["m0"], st["v0"], s, lr, b1, b2, eps, st["max_norm"], W)
        assert error_stats(st["torch"]["p"], p64, scale=st["scales"]["p"])["max_ulp"] <= bound["p"]
        assert error_stats(st["torch"]["m"], m64, scale=st["scales"]["m"])["max_ulp"] <= bound["m"]
        assert error_stats(st["torch"]["v"], v64, scale=st["scales"]["v"])["max_ulp"] <= bound["v"]
        assert abs(n64 - st["r64"]["norm"]) <= 1e-12 * n64
    record(f"hp {name}: torch vs float64, largest over {H.N_STEPS} steps (ulp)", worst)

    # the sensitivity guard, per field the case moves off its default, pooled over the steps
    fields = dict(H.CASES[name][0])
    fields.pop("update_target_every", None)
    if H.CASES[name][1] == "edge":
        fields["max_norm"] = None
    for field, value in fields.items():
        for q in _field_targets(field, value):
            moved = total = 0.0
            for s, st in enumerate(steps):
                alt = dict(hp)
                alt[field] = H.DEFAULTS[field]
                mn = alt["max_norm"] if field == "max_norm" else st["max_norm"]
                r_alt = H.adam_ref64(st["p0"], st["g"], st["m0"], st["v0"],
                                     H.adam_scalars(alt["lr"], alt["betas"][0], alt["betas"][1], s), alt["adam_eps"],
                                     mn, alt["world_size"])
                moved += H.guard_fraction(st["r64"], r_alt, st["scales"], bound[q], q)
                total += 1.0
            frac = moved / total
            record(f"hp {name}: guard, {field} -> {q}: fraction of elements moved by > 10x the bound", {"fraction": frac})
            assert frac > 0.01, (name, field, q, frac)


def test_case_conditions(p_init):
    """What the cases claim of their own inputs: adam_eps = 1e-3 dominates sqrt(v_hat) on more than
    1 % of the elements and 1e-12 is negligible; max_norm = 1e-3 is below every step's norm and 1e3
    above; the edge case's coefficient falls on both sides of 1 within 1 %; adam_eps = 0 has no
    element below 1e-6; world_size = 2 halves a gradient whose norm lies between 1 and 2."""
    for name, want in (("adam_eps=1e-3", "dominates"), ("adam_eps=1e-12", "negligible")):
        hp, steps = walk(name, p_init)
        for st in steps:
            root = (st["r64"]["v"] / st["sc"]["bc2"]).sqrt()
            if want == "dominates":
                assert float((hp["adam_eps"] > root).double().mean()) > 0.01
            else:
                nz = root[root > 0]
                assert float((hp["adam_eps"] < 0.01 * nz).double().mean()) > 0.99
    for name in ("max_norm=1e-3", "max_norm=1e3", "max_norm=edge", "world_size=2"):
        hp, steps = walk(name, p_init)
        for s, st in enumerate(steps):
            coef = st["max_norm"] / (st["r64"]["norm"] + 1e-6)
            if name == "max_norm=1e-3":
                assert coef < 1.0
            elif name == "max_norm=1e3":
                assert coef > 1.0
            elif name == "max_norm=edge":
                assert (1.0 < coef < 1.01) if s % 2 == 0 else (0.99 < coef < 1.0)
            else:
                assert 0.5 < st["r64"]["norm"] < 1.0 and 1.0 < 2.0 * st["r64"]["norm"] < 2.0
    for s in range(H.N_STEPS):
        g = H.synthetic_grad("adam_eps=0", s)
        assert float(g.abs().min()) >= 1e-6
        z = H.synthetic_grad("lr=0", s)
        assert 0.02 < float((z == 0).double().mean()) < 0.08


def test_transition_restatement_matches_torch_away_from_the_transition():
    """adam_ref64 with a mixture of scalars is the transition step's reference on the GPU; with the
    scalars of one set of hyper-parameters it is the plain step checked above, and the product of the
    betas in force equals beta**step while the betas never change (the running double product is
    within step * 2^-53 relative of it)."""
    for b in (0.9, 0.999, 0.5, 0.9999):
        prod = 1.0
        for s in range(1, 3001):
            prod *= b
            if s in (1, 2, 10, 100, 1000, 3000):
                assert abs(prod - b ** s) <= s * 2.0 ** -53 * b ** s + 5e-324
