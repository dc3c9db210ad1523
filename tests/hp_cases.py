"""Optimizer hyper-parameter cases shared by tests/test_hp_reference_host.py (CPU) and
tests/test_gpu_hp_reference.py (GPU): the case table, the seeded synthetic gradients, a float64
restatement of clip_grad_norm_ + torch.optim.Adam from the fp32 inputs, an fp32 NumPy restatement
of the same (every operation rounded to fp32: it measures the fp32 rounding noise a correct fp32
implementation may show), the scales the errors are measured at, and the sensitivity guard.

Bounds (fixed before any GPU run): per quantity, the larger of the project's bound
(tests/test_gpu_parity_large.py: m 8 ulp and v 16 ulp of their terms, p 4 ulp of max(|p|, lr), norm
8 ulp) and 2x the fp32 restatement's largest distance to float64 on the same inputs, over the steps
of the case.  The 2x allows for the kernel's v_sqrt_f32 / v_rcp_f32 at <= 1 ulp each where the
restatement's square root and divisions are correctly rounded.

Scales: m at b1 * |m0| + (1 - b1) * |g_clipped| (its terms), and at max(|m0|, |g_clipped|) when
beta1 < 0.5 (torch's lerp_ switches formula at weight 0.5; the kernel's m + w (g - m) then rounds at
|m0|); v at its terms; p at max(|p0|, |update|, lr) (with a small beta2, m / sqrt(v) is not bounded
by 1).
"""
import math

import numpy as np
import torch

N_PARAMS = 1673
N_STEPS = 6
DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8, max_norm=1.0, world_size=1, update_target_every=200)
PROJECT_ULP = dict(m=8.0, v=16.0, p=4.0, norm=8.0)
ALL_AT_ONCE = dict(lr=3e-4, betas=(0.5, 0.9), adam_eps=1e-3, max_norm=0.05, update_target_every=1)

# name -> (hyper-parameters that differ from DEFAULTS, gradient kind)
# gradient kinds: "std" (below), "nonzero" (no exact zeros, |g| >= 1e-6: adam_eps = 0), "norm1.5"
# (std, rescaled to a norm of 1.5: world_size = 2 then halves an unclipped gradient where
# world_size = 1 clips it, and a division by W after the clip would clip it too), "edge" (std, with
# max_norm set per step to 1.005x / 0.995x the step's own norm: the clamp's two sides)
CASES = {
    "lr=3e-3": (dict(lr=3e-3), "std"),
    "lr=1e-5": (dict(lr=1e-5), "std"),
    "lr=0": (dict(lr=0.0), "std"),
    "betas=(0.5,0.999)": (dict(betas=(0.5, 0.999)), "std"),
    "betas=(0.9,0.9)": (dict(betas=(0.9, 0.9)), "std"),
    "betas=(0.0,0.999)": (dict(betas=(0.0, 0.999)), "std"),
    "betas=(0.9,0.0)": (dict(betas=(0.9, 0.0)), "std"),
    "betas=(0.99,0.9999)": (dict(betas=(0.99, 0.9999)), "std"),
    "adam_eps=1e-3": (dict(adam_eps=1e-3), "std"),
    "adam_eps=1e-12": (dict(adam_eps=1e-12), "std"),
    "adam_eps=0": (dict(adam_eps=0.0), "nonzero"),
    "max_norm=1e-3": (dict(max_norm=1e-3), "std"),
    "max_norm=1e3": (dict(max_norm=1e3), "std"),
    "max_norm=edge": (dict(), "edge"),
    "world_size=2": (dict(world_size=2), "norm1.5"),
    "all at once": (dict(ALL_AT_ONCE), "std"),
}


def case_hp(name):
    hp = dict(DEFAULTS)
    hp.update(CASES[name][0])
    return hp


def synthetic_grad(name, step, kind=None):
    """The case's gradient of optimizer step `step` (0-based), fp32 [N_PARAMS]: randn * 10**U(-6, 0.5)
    per element, 5 % exact zeros (none for kind "nonzero"), a fresh draw every step."""
    kind = CASES[name][1] if kind is None else kind
    seed = 1000 * (sorted(CASES).index(name) + 1 if name in CASES else 97) + step
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(N_PARAMS, generator=gen, dtype=torch.float64)
    g = g * 10.0 ** (torch.rand(N_PARAMS, generator=gen, dtype=torch.float64) * 6.5 - 6.0)
    zero = torch.rand(N_PARAMS, generator=gen) < 0.05
    if kind == "nonzero":
        sign = torch.where(g < 0, -1.0, 1.0).double()
        g = sign * g.abs().clamp_min(1.001e-6)   # still >= 1e-6 once rounded to fp32
    else:
        g = torch.where(zero, torch.zeros_like(g), g)
    if kind == "norm1.5":
        g = g * (1.5 / float(g.norm()))
    return g.to(torch.float32)


def step_max_norm(name, step, g, world_size=1):
    """max_norm of the case at this step: the case's own, or for "edge" 1.005x (even steps: the
    coefficient is above 1 and clamps, no clip) / 0.995x (odd steps: clips by 0.995) the norm."""
    if CASES[name][1] != "edge":
        return case_hp(name)["max_norm"]
    norm = float((g.double() / world_size).norm())
    return float(np.float32(norm * (1.005 if step % 2 == 0 else 0.995)))


def f32(x):
    return float(np.float32(x))


def adam_scalars(lr, b1, b2, step0):
    """The step's scalars as torch.optim.Adam forms them (_single_tensor_adam, Python floats):
    step_size = lr / (1 - beta1^t), bias_correction2 = 1 - beta2^t, t = step0 + 1."""
    t = step0 + 1
    return dict(step_size=lr / (1.0 - b1 ** t), bc2=1.0 - b2 ** t, one_m_b1=1.0 - b1, b2=b2, one_m_b2=1.0 - b2)


def adam_ref64(p0, g, m0, v0, sc, eps, max_norm, world_size=1):
    """clip_grad_norm_ + one Adam step in float64 from the fp32 inputs.  ``sc``: the step's scalars
    (adam_scalars, or any mixture of them: the transition step after set_hp); those that torch and
    the kernel hold as fp32 (the lerp weight, beta2, 1 - beta2, eps, the step size) enter as their
    fp32 values.  Returns dict(p, m, v, norm, gc, update)."""
    p0, g = p0.double(), g.double()
    m0 = torch.zeros_like(p0) if m0 is None else m0.double()
    v0 = torch.zeros_like(p0) if v0 is None else v0.double()
    if world_size > 1:
        g = g * f32(1.0 / world_size)
    norm = float(g.norm())
    gc = g * min(1.0, max_norm / (norm + 1e-6))
    m = m0 + f32(sc["one_m_b1"]) * (gc - m0)
    v = f32(sc["b2"]) * v0 + f32(sc["one_m_b2"]) * gc * gc
    update = f32(sc["step_size"]) * m / (v.sqrt() / math.sqrt(sc["bc2"]) + f32(eps))
    return dict(p=p0 - update, m=m, v=v, norm=norm, gc=gc, update=update)


def adam_np32(p0, g, m0, v0, sc, eps, max_norm, world_size=1):
    """torch's clip_grad_norm_ + _single_tensor_adam restated in NumPy with every operation rounded
    to fp32 (square root and divisions correctly rounded) and the scalars formed in double as torch
    forms them.  Used only to measure fp32 rounding noise against adam_ref64."""
    F = np.float32
    p, g = p0.numpy().astype(F), g.numpy().astype(F)
    m = np.zeros_like(p) if m0 is None else m0.numpy().astype(F)
    v = np.zeros_like(p) if v0 is None else v0.numpy().astype(F)
    if world_size > 1:
        g = g * F(1.0 / world_size)
    norm = np.sqrt(np.sum(g * g, dtype=F))
    coef = F(max_norm) / (norm + F(1e-6))
    g = g * (coef if coef < F(1.0) else F(1.0))
    w = F(sc["one_m_b1"])
    m = m + w * (g - m) if w < F(0.5) else g - (g - m) * (F(1.0) - w)   # lerp_
    v = v * F(sc["b2"])
    v = v + (F(sc["one_m_b2"]) * g) * g                                   # addcmul_
    denom = np.sqrt(v) / F(math.sqrt(sc["bc2"])) + F(eps)
    p = p + (F(-sc["step_size"]) * m) / denom                             # addcdiv_
    return dict(p=torch.from_numpy(p), m=torch.from_numpy(m), v=torch.from_numpy(v), norm=float(norm))


def scales(p0, m0, v0, r64, sc, lr):
    """The magnitudes the errors are measured at (module docstring), from the float64 step r64."""
    m0 = torch.zeros_like(r64["m"]) if m0 is None else m0.double()
    v0 = torch.zeros_like(r64["v"]) if v0 is None else v0.double()
    gc = r64["gc"]
    b1 = 1.0 - sc["one_m_b1"]
    m_s = b1 * m0.abs() + sc["one_m_b1"] * gc.abs()
    if b1 < 0.5:
        m_s = torch.maximum(m0.abs(), gc.abs())
    v_s = sc["b2"] * v0.abs() + sc["one_m_b2"] * gc * gc
    p_s = torch.maximum(torch.maximum(p0.double().abs(), r64["update"].abs()), torch.full_like(gc, lr))
    return dict(m=m_s, v=v_s, p=p_s)


def ulp_errors(got, r64, sc_):
    """Largest error of got's p, m, v, norm against the float64 step, in fp32 ulps of the scales."""
    from tests.conftest import error_stats
    out = {k: error_stats(got[k], r64[k], scale=sc_[k])["max_ulp"] for k in ("p", "m", "v")}
    out["norm"] = error_stats(torch.tensor([got["norm"]]), torch.tensor([r64["norm"]]))["max_ulp"]
    return out


def bounds_from_noise(noise):
    """Per quantity: max(the project's bound, 2x the fp32 restatement's largest error), in ulps."""
    return {k: max(PROJECT_ULP[k], 2.0 * noise[k]) for k in PROJECT_ULP}


def guard_fraction(r_case, r_default, sc_, bound_ulp, quantity):
    """Sensitivity guard: the fraction of `quantity`'s elements on which the reference at the case's
    value and the reference at the default differ by more than 10x the asserted bound."""
    from tests.conftest import fp32_ulp
    b = r_case[quantity]
    ref = torch.maximum(b.abs(), sc_[quantity])
    tol = 10.0 * bound_ulp * fp32_ulp(ref)
    return float(((r_case[quantity] - r_default[quantity]).abs() > tol).double().mean())


class CtrlModel:
    """What the control block holds of the optimizer, restated on the host: the running products of
    the betas each applied step carried, and the scalars of the NEXT step, formed after every step
    from the hyper-parameters of the launch that applied it (swarm_ctrl, include/swarm_hip.h).
    ``step(hp)`` returns the scalars the step launched with ``hp`` computes with: step size, bias
    correction 2 and 1 - beta from the launch before it; v's decay beta2 from ``hp`` itself.  While
    the betas never change the products are beta**step and this is torch.optim.Adam's step; after
    set_hp(betas=...) the bias corrections are 1 - the product of the betas in force at each step
    (by design; torch's would be 1 - new_beta**step), and the first step launched with new values
    is a mixture: old lr, old 1 - beta and old bias corrections, new decay of v."""

    def __init__(self, hp):
        self.p1 = self.p2 = 1.0
        self._store(hp)

    def _store(self, hp):
        b1, b2 = hp["betas"]
        self.next = dict(step_size=hp["lr"] / (1.0 - self.p1 * b1), bc2=1.0 - self.p2 * b2, one_m_b1=1.0 - b1,
                         one_m_b2=1.0 - b2)

    def step(self, hp):
        sc = dict(self.next, b2=hp["betas"][1])
        self.p1 *= hp["betas"][0]
        self.p2 *= hp["betas"][1]
        self._store(hp)
        return sc
