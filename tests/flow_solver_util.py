"""Float64 reference of the flow head's higher-order integrators (fv_head_set_flow_solver; tests only), built on flow_util / rtc_util / flow_prefix_util
without editing them: the tableaux, the plain, guided and prefix Runge-Kutta samplers with their fp32 CPU emulations (used ONLY to calibrate the GPU
samplers' bar), and the cases host and GPU tests share.

The scheme (explicit Runge-Kutta methods whose stage j + 1 depends on stage j only).  Within a step from t_i to t_i + h, h = -1 / N, x0 the step's start and
k_j = v(x_j, t_i + c_j h):      x_1 = x0      x_{j+1} = x0 + (a_{j+1} h) k_j      S = sum_j b_j k_j      x <- x0 + h S
Scalars follow flow_util.euler_sample's rule: the stage times 1 - (i + c_j) / N are the fp32 values the library hands its kernels; the float64 reference
keeps a h, b and h in double (as euler_sample keeps dt), the emulation rounds them to fp32 once (as the library does)."""
from __future__ import annotations

import functools

import numpy as np
import torch

import flow_prefix_util as pu
import flow_util as fu
import rtc_util as ru

# name -> (c, a, b): stage times, a[j] the coefficient that forms stage j + 1's x from k_j, the weights of the sum
TABLEAUX = {
    "euler": ((0.0,), (), (1.0,)),
    "midpoint": ((0.0, 0.5), (0.5,), (0.0, 1.0)),
    "heun": ((0.0, 1.0), (1.0,), (0.5, 0.5)),
    "rk4": ((0.0, 0.5, 0.5, 1.0), (0.5, 0.5, 1.0), (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)),
}
STAGES = {k: len(v[0]) for k, v in TABLEAUX.items()}
HIGHER = ("midpoint", "heun", "rk4")
SAMPLE_OFFSET_ERROR = 1 << 63      # action_error_per_dim's noise: the flow seed at this offset (a range of its own)


def stage_time(i: int, c: float, N: int) -> np.float32:
    """1 - (i + c) / N in double, rounded once: a stage with c = 1 sees exactly the bits of t_{i + 1}"""
    return np.float32(1.0 - (float(i) + c) / float(N))


def integrate(x, N: int, solver: str, vel, *, fp32: bool = False, live=None):
    """the scheme on a velocity vel(x, t) -> k, t a python float holding the fp32 stage time.  fp32: every scalar rounded once to fp32 and every operation in
    fp32 (x is then a float32 tensor).  live (bool, x's shape): elements outside it are never updated (the prefix sampler's pinned steps)"""
    c, a, b = TABLEAUX[solver]
    h = -1.0 / N
    r = (lambda v: float(np.float32(v))) if fp32 else (lambda v: v)
    for i in range(N):
        x0, S = x, None
        for j in range(len(c)):
            k = vel(x, float(stage_time(i, c[j], N)))
            S = r(b[j]) * k if S is None else S + r(b[j]) * k
            new = x0 + r(h) * S if j + 1 == len(c) else x0 + r(a[j] * h) * k
            x = new if live is None else torch.where(live, new, x0)
    return x


def _prep(p, pooled, states, dtype, state_norm):
    p = {k: v.to(dtype) for k, v in p.items()}
    pooled, states = pooled.to(dtype), states.to(dtype)
    if state_norm is not None:
        if dtype == torch.float32:
            states = (states - state_norm[0].float()) * (1.0 / (state_norm[1].float() + np.float32(state_norm[2])))
        else:
            states = (states - state_norm[0].double()) / (state_norm[1].double() + state_norm[2])
    return p, pooled, states


def _phi(B: int, t: float, E: int, fp32: bool):
    if fp32:
        a = torch.from_numpy(fu.flow_freqs(E)) * t
        return torch.cat([a.sin(), a.cos()]).expand(B, -1)
    return fu.phi_exact(np.full(B, np.float32(t)), E)


def _finish(x, action_norm, dtype):
    return x if action_norm is None else x * action_norm[1].to(dtype) + action_norm[0].to(dtype)


# ------------------------------------------------------------------------------------------------------------------ the plain sampler
def rk_sample(p: dict, pooled, states, noise, N: int, E: int, solver: str = "euler", *, state_norm=None, action_norm=None, field=None) -> torch.Tensor:
    """float64; flow_util.euler_sample's arguments and options.  solver = "euler" IS euler_sample, operation for operation"""
    p, pooled, states = _prep(p, pooled, states, torch.float64, state_norm)
    x = noise.double().clone()
    vel = field if field is not None else (lambda x_, t: fu.velocity(p, pooled, states, x_, _phi(x_.shape[0], t, E, False)))
    return _finish(integrate(x, N, solver, vel), action_norm, torch.float64)


def rk_sample_fp32(p: dict, pooled, states, noise, N: int, E: int, solver: str = "euler", *, state_norm=None, action_norm=None, field=None) -> torch.Tensor:
    """the same sampler with every operation in fp32 on the CPU (flow_util.euler_sample_fp32's recipe): the yardstick of the GPU sampler's bar"""
    p, pooled, states = _prep(p, pooled, states, torch.float32, state_norm)
    x = noise.float().clone()
    vel = field if field is not None else (lambda x_, t: fu.velocity(p, pooled, states, x_, _phi(x_.shape[0], t, E, True)))
    return _finish(integrate(x, N, solver, vel, fp32=True), action_norm, torch.float32)


# ------------------------------------------------------------------------------------------------------------------ the guided sampler
def guidance_k(t: float, beta: float) -> float:
    """rtc_util.guidance_k for a STAGE time: beta at t = 1 and, the ratio being unbounded there, at t = 0 (the last stage of the last step of Heun and RK4)"""
    return float(beta) if t <= 0.0 else ru.guidance_k(t, beta)


def guided_rk(p: dict, pooled, states, noise, N: int, E: int, Y, W, beta: float, solver: str, *, state_norm=None, action_norm=None, fp32: bool = False):
    """-> (actions, chunk), rtc_util.guided_euler's arguments: every stage evaluates the corrected velocity v' = v - k (omega - t J^T omega) with the stage's
    t and k.  solver = "euler" is guided_euler"""
    dt_ = torch.float32 if fp32 else torch.float64
    p, pooled, states = _prep(p, pooled, states, dt_, state_norm)
    Y, W = Y.to(dt_), W.to(dt_)
    live = W > 0

    def vel(x, t):
        k = guidance_k(t, beta)
        k = float(np.float32(k)) if fp32 else k
        x = x.detach().requires_grad_(True)
        v = fu.velocity(p, pooled, states, x, _phi(x.shape[0], t, E, fp32))
        with torch.no_grad():
            omega = torch.where(live, W * (Y - (x - t * v)), torch.zeros_like(x))
        jt, = torch.autograd.grad(v, x, omega)
        return (v - k * (omega - t * jt)).detach()

    chunk = integrate(noise.to(dt_).clone(), N, solver, vel, fp32=fp32)
    return _finish(chunk, action_norm, dt_), chunk


# ------------------------------------------------------------------------------------------------------------------ the prefix sampler
def prefix_rk(p: dict, pooled, states, noise, prev, delays, shift: int, N: int, E: int, K: int, D: int, solver: str, *, state_norm=None, action_norm=None,
              fp32: bool = False):
    """-> (actions, chunk), flow_prefix_util.prefix_euler_sample's arguments: a pinned element is never updated, at any stage"""
    dt_ = torch.float32 if fp32 else torch.float64
    p, pooled, states = _prep(p, pooled, states, dt_, state_norm)
    B, da = noise.shape
    A = da // K
    pin = pu.pinned_steps(delays, D, K, shift)
    m = torch.from_numpy(pu.mask_ref(pin, K)).to(dt_)
    live = ~(m.bool().repeat_interleave(A, dim=1))
    x = noise.to(dt_).clone()
    pv = torch.as_tensor(prev).to(dt_)
    for b in range(B):
        n = int(pin[b]) * A
        x[b, :n] = pv[b, shift * A:shift * A + n]
    vel = lambda x_, t: pu.velocity(p, pooled, states, x_, _phi(B, t, E, fp32), m)      # noqa: E731
    chunk = integrate(x, N, solver, vel, fp32=fp32, live=live)
    return _finish(chunk, action_norm, dt_), chunk


# ------------------------------------------------------------------------------------------------------------------ the linear-Gaussian toy of tests/test_flow_host.py
def toy():
    """-> (field, eps, exact): a ~ N(m, s^2 I), eps ~ N(0, I); the exact flow maps x_1 = eps to m + s eps (same m, s and seed as
    test_reference_sampler_error_falls_as_one_over_n)"""
    m, s = torch.tensor([0.7, -1.2, 0.3]).double(), 0.5
    eps = torch.randn(64, 3, generator=torch.Generator().manual_seed(0)).double()

    def field(x, t):
        return -m + (t - (1 - t) * s * s) / (t * t + (1 - t) ** 2 * s * s) * (x - (1 - t) * m)

    return field, eps, m + s * eps


def toy_error(solver: str, N: int) -> float:
    field, eps, exact = toy()
    out = rk_sample({}, torch.zeros(64, 1), torch.zeros(64, 1), eps, N, 2, solver, field=field)
    return float((out - exact).norm() / exact.norm())


# ------------------------------------------------------------------------------------------------------------------ the cases host and GPU tests share
HEADS, BATCHES, STEPS = ("awkward", "larger"), fu.SAMPLER_BATCHES, (1, 4)
PREFIX_SHIFTS = lambda K: (0, K // 3)      # noqa: E731
GUIDED_CONFIGS = (("exp", "d0"), ("zeros", "d0"), ("exp", "third"), ("zeros", "third"))      # (schedule, rtc_util.rtc_config's name)


def mixed_delays(B: int, D: int) -> np.ndarray:
    """0, 1 and D mixed within a batch; row 0 pins D steps"""
    return np.array([(D, 0, 1)[r % 3] for r in range(B)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def prefix_case(name: str, B: int) -> dict:
    """flow_prefix_util.prefix_case with this file's delays (a copy: the cached case stays unchanged)"""
    c = dict(pu.prefix_case(name, B))
    c["delays"] = mixed_delays(B, c["D"])
    return c


@functools.lru_cache(maxsize=None)
def plain_refs(name: str, B: int, N: int, io: bool, solver: str):
    """-> (float64 reference, the fp32 emulation's distance from it in the sampler's measure)"""
    c = fu.sampler_case(name, B)
    args, kw = (c["p"], c["pooled"], c["states"], c["noise"], N, c["dims"][6], solver), ru.io_kwargs(c, io)
    ref = rk_sample(*args, **kw)
    return ref, fu.worst_row_vs_rms(rk_sample_fp32(*args, **kw), ref)


@functools.lru_cache(maxsize=None)
def prefix_refs(name: str, B: int, N: int, io: bool, shift: int, solver: str):
    """-> (actions64, chunk64, emulation distance of actions, of chunk)"""
    c = prefix_case(name, B)
    K, E = c["dims"][4], c["dims"][6]
    args = (c["p"], c["pooled"], c["states"], c["noise"], c["prev"], c["delays"], shift, N, E, K, c["D"], solver)
    act, chunk = prefix_rk(*args, **ru.io_kwargs(c, io))
    act32, chunk32 = prefix_rk(*args, **ru.io_kwargs(c, io), fp32=True)
    return act, chunk, fu.worst_row_vs_rms(act32, act), fu.worst_row_vs_rms(chunk32, chunk)


@functools.lru_cache(maxsize=None)
def guided_refs(name: str, B: int, N: int, io: bool, schedule: str, which: str, solver: str):
    """-> (actions64, chunk64, emulation distance of actions, of chunk)"""
    c = ru.rtc_case(name, B)
    K, A, E = c["dims"][4], c["dims"][5], c["dims"][6]
    d, s, shift = ru.rtc_config(K, which)
    Y, W = ru.targets(c["prev"], ru.prefix_weights_ref(K, d, s, schedule), K, A, shift)
    args = (c["p"], c["pooled"], c["states"], c["noise"], N, E, Y, W, ru.BETA, solver)
    act, chunk = guided_rk(*args, **ru.io_kwargs(c, io))
    act32, chunk32 = guided_rk(*args, **ru.io_kwargs(c, io), fp32=True)
    return act, chunk, fu.worst_row_vs_rms(act32, act), fu.worst_row_vs_rms(chunk32, chunk)


def plain_cases():
    return [(n, B, N, io, s) for n in HEADS for B in BATCHES for s in HIGHER for N in STEPS for io in (False, True)]


def prefix_cases():
    return [(n, B, N, io, sh, s) for n in HEADS for B in BATCHES for s in HIGHER for N in STEPS for io in (False, True) for sh in PREFIX_SHIFTS(fu.DIMS[n][4])]


def guided_cases():
    return [(n, B, N, io, sched, which, s) for n in HEADS for B in BATCHES for s in HIGHER for N in STEPS for io in (False, True) for sched, which in GUIDED_CONFIGS]
