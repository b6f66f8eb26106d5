"""Float64 reference of the guided (real-time chunking) Euler sampler (tests only), built on flow_util.velocity with torch.autograd.grad for J^T omega; its
fp32 CPU emulation (used ONLY to calibrate the GPU sampler's bar); the closed form of the prefix weights; the cases host and GPU tests share.

Convention (flow_util's): x_t = t eps + (1 - t) a, v ~ eps - a, sampling from t = 1 down to 0 with x <- x + dt v, dt = -1 / N.  Per step, with W the
per-element weights (w[k] broadcast over the A dimensions of step k, 0 beyond the shift and in unguided rows) and Y the shifted previous chunk:
    a^ = x - t v      omega = W (Y - a^), SELECTED to 0 where W == 0      g = omega - t J^T omega      k = beta at t = 1, else min(beta, ((1-t)^2 + t^2) / ((1-t) t))
    v' = v - k g      x <- x + dt v'"""
from __future__ import annotations

import functools

import numpy as np
import torch

import flow_util as fu


# ------------------------------------------------------------------------------------------------------------------ weights
def prefix_weights_ref(K: int, d: int, s: int, schedule: str) -> np.ndarray:
    """(K,) float64, the closed form: 1 on k < d, 0 from K - s on, between them c (e^c - 1) / (e - 1) ("exp"), c ("linear"), 1 ("ones"), 0 ("zeros") with
    c = (K - s - k) / (K - s - d + 1)"""
    k = np.arange(K, dtype=np.float64)
    c = (K - s - k) / (K - s - d + 1.0)
    mid = {"exp": c * (np.exp(c) - 1.0) / (np.e - 1.0), "linear": c, "ones": np.ones(K), "zeros": np.zeros(K)}[schedule]
    return np.where(k < d, 1.0, np.where(k >= K - s, 0.0, mid))


def guidance_k(t: float, beta: float) -> float:
    """in double, from the fp32-rounded t the sampler is handed"""
    return float(beta) if t == 1.0 else min(float(beta), ((1.0 - t) ** 2 + t * t) / ((1.0 - t) * t))


def targets(prev, w, K: int, A: int, shift: int, row_mask=None):
    """-> (Y, W) (B, K A) float64: Y[b][k] = prev[b][k + shift] (0 where there is none), W = w[k] where k + shift < K and the row is guided, else 0"""
    prev = torch.as_tensor(prev).double()
    B = prev.shape[0]
    Y = torch.zeros(B, K, A, dtype=torch.float64)
    W = torch.zeros(B, K, A, dtype=torch.float64)
    n = K - shift
    if n > 0:
        Y[:, :n] = prev.view(B, K, A)[:, shift:]
        W[:, :n] = torch.as_tensor(np.asarray(w, dtype=np.float32).astype(np.float64))[:n].view(1, n, 1)      # (the weights are uploaded as fp32)
    if row_mask is not None:
        W = W * (torch.as_tensor(row_mask).view(B, 1, 1) != 0).double()
    return Y.view(B, K * A), W.view(B, K * A)


# ------------------------------------------------------------------------------------------------------------------ the guided sampler
def guided_euler(p: dict, pooled, states, noise, N: int, E: int, Y, W, beta: float, *, state_norm=None, action_norm=None, fp32: bool = False):
    """-> (actions, chunk): chunk is the final normalised x_0, actions its un-normalisation (the same tensor without action_norm).  fp32 = False: float64
    throughout.  fp32 = True: every operation in fp32 on the CPU (euler_sample_fp32's recipe, k rounded once, autograd in fp32): the emulation."""
    dt_ = torch.float32 if fp32 else torch.float64
    p = {k: v.to(dt_) for k, v in p.items()}
    pooled, states, x = pooled.to(dt_), states.to(dt_), noise.to(dt_).clone()
    Y, W = Y.to(dt_), W.to(dt_)
    live = W > 0
    if state_norm is not None:
        if fp32:
            states = (states - state_norm[0].float()) * (1.0 / (state_norm[1].float() + np.float32(state_norm[2])))
        else:
            states = (states - state_norm[0].double()) / (state_norm[1].double() + state_norm[2])
    ts = fu.step_times(N)
    dt = float(np.float32(-1.0 / N)) if fp32 else -1.0 / N
    wfreq = torch.from_numpy(fu.flow_freqs(E))
    for i in range(N):
        t = float(ts[i])
        k = guidance_k(t, beta)
        if fp32:
            k = float(np.float32(k))
            a = wfreq * t
            phi = torch.cat([a.sin(), a.cos()]).expand(x.shape[0], -1)
        else:
            phi = fu.phi_exact(np.full(x.shape[0], ts[i]), E)
        x = x.detach().requires_grad_(True)
        v = fu.velocity(p, pooled, states, x, phi)
        with torch.no_grad():
            omega = torch.where(live, W * (Y - (x - t * v)), torch.zeros_like(x))
        jt, = torch.autograd.grad(v, x, omega)
        x = (x + dt * (v - k * (omega - t * jt))).detach()
    chunk = x
    if action_norm is not None:
        x = x * action_norm[1].to(dt_) + action_norm[0].to(dt_)
    return x, chunk


def vjp_ref(p: dict, pooled, states, x, t: float, omega, E: int, fp32: bool = False):
    """-> (v, J^T omega) of one step at time t (a float that fp32 holds exactly)"""
    dt_ = torch.float32 if fp32 else torch.float64
    p = {k: v.to(dt_) for k, v in p.items()}
    x = x.to(dt_).clone().requires_grad_(True)
    if fp32:
        a = torch.from_numpy(fu.flow_freqs(E)) * t
        phi = torch.cat([a.sin(), a.cos()]).expand(x.shape[0], -1)
    else:
        phi = torch.from_numpy(fu.phi_ref(np.full(x.shape[0], t, dtype=np.float32), fu.flow_freqs(E)))
    v = fu.velocity(p, pooled.to(dt_), states.to(dt_), x, phi)
    jt, = torch.autograd.grad(v, x, omega.to(dt_))
    return v.detach(), jt


# ------------------------------------------------------------------------------------------------------------------ shared cases
BETA = 5.0
RTC_CONFIGS = ("d0", "d1", "third")      # (d, s, shift) = (0, 1, 1), (1, 1, 1), (K/3, K/3, K/3)


def rtc_config(K: int, which: str):
    third = max(1, K // 3)
    return {"d0": (0, 1, 1), "d1": (1, 1, 1), "third": (third, third, third)}[which]


@functools.lru_cache(maxsize=None)
def rtc_case(name: str, B: int) -> dict:
    """flow_util.sampler_case plus a previous chunk: the float64 unguided sample of ANOTHER start noise for the same observation (a plausible chunk of the
    same distribution, in normalised space), rounded to fp32.  Cached: computed once per session and left unchanged."""
    case = dict(fu.sampler_case(name, B))
    E, da = case["dims"][6], case["dims"][4] * case["dims"][5]
    g = torch.Generator().manual_seed(4242 + B)
    other = torch.randn(B, da, generator=g)
    case["prev"] = fu.euler_sample(case["p"], case["pooled"], case["states"], other, 10, E).float()
    return case


def io_kwargs(case: dict, io: bool) -> dict:
    st = case["stats"]
    return dict(state_norm=(st["state_mean"], st["state_std"], 1e-8), action_norm=(st["action_mean"], st["action_std"])) if io else {}


@functools.lru_cache(maxsize=None)
def guided_refs(name: str, B: int, N: int, io: bool, schedule: str, which: str):
    """-> (actions64, chunk64, emulation distance of actions, of chunk) for one GPU sampler case"""
    case = rtc_case(name, B)
    K, A, E = case["dims"][4], case["dims"][5], case["dims"][6]
    d, s, shift = rtc_config(K, which)
    Y, W = targets(case["prev"], prefix_weights_ref(K, d, s, schedule), K, A, shift)
    args = (case["p"], case["pooled"], case["states"], case["noise"], N, E, Y, W, BETA)
    act, chunk = guided_euler(*args, **io_kwargs(case, io))
    act32, chunk32 = guided_euler(*args, **io_kwargs(case, io), fp32=True)
    return act, chunk, fu.worst_row_vs_rms(act32, act), fu.worst_row_vs_rms(chunk32, chunk)


def prefix_distance(chunk, Y, d: int, A: int) -> float:
    """max |chunk - Y| over the hard prefix (the first d steps)"""
    return float((torch.as_tensor(chunk).double()[:, :d * A] - Y[:, :d * A]).abs().max())
