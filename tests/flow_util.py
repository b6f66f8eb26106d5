"""Float64 reference of the flow-matching action head (tests only): noising, the sinusoidal time embedding, the velocity network as float64 torch (autograd
works through it), the Euler sampler, an fp32 CPU emulation of the sampler (used ONLY to calibrate the GPU sampler's bar) and the draw stream.

Convention (pi0 / SmolVLA, normalised action space):  x_t = t eps + (1 - t) a,  u = eps - a,  sampling from x_1 = eps with x <- x + dt v, dt = -1 / N.
    cat = [ pooled | state branch | x_t | phi(t) ],  phi(t) = [ sin(w_j t) | cos(w_j t) ],  w_j = 2 pi / p_j,  p_j geometric from min_period to max_period.
The draws: Philox4x32-10 (tests/augment_util.py's, pinned by the Random123 known answers) with key = seed ^ (FLOW_KEY_LO, FLOW_KEY_HI) and counter
(group, row, offset lo, offset hi): group 0 is the row's t, group 1 + i // 4 holds the normals of elements 4 (i // 4) .. + 3 (two Box-Muller pairs)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from augment_util import philox4x32_10

FLOW_KEY_LO, FLOW_KEY_HI = 0x464C4F57, 0x4D415443
MIN_PERIOD, MAX_PERIOD = 4e-3, 4.0
LN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------ time embedding and noising
def flow_freqs(E: int, min_period: float = MIN_PERIOD, max_period: float = MAX_PERIOD) -> np.ndarray:
    """(E / 2,) float32: w_j = 2 pi / p_j computed in float64 FROM THE fp32 PERIODS the library is handed, rounded once (what fv_head_set_flow uploads)"""
    half = E // 2
    lo, hi = float(np.float32(min_period)), float(np.float32(max_period))
    frac = np.arange(half, dtype=np.float64) / (half - 1) if half > 1 else np.zeros(1)
    return (2.0 * np.pi / (lo * (hi / lo) ** frac)).astype(np.float32)


def phi_args(t, freqs32: np.ndarray) -> np.ndarray:
    """(B, E / 2) float32: the fp32 product w_j t the device forms (one rounding)"""
    return (np.asarray(t, dtype=np.float32)[:, None] * freqs32[None, :]).astype(np.float32)


def phi_ref(t, freqs32: np.ndarray) -> np.ndarray:
    """(B, E) float64: sin | cos of the fp32-rounded argument, evaluated in float64"""
    a = phi_args(t, freqs32).astype(np.float64)
    return np.concatenate([np.sin(a), np.cos(a)], axis=1)


def phi_exact(t, E: int, min_period: float = MIN_PERIOD, max_period: float = MAX_PERIOD) -> torch.Tensor:
    """(B, E) float64 torch, everything in float64 (the reference sampler's own embedding)"""
    w = torch.from_numpy(flow_freqs(E, min_period, max_period).astype(np.float64))
    a = torch.as_tensor(t, dtype=torch.float64).reshape(-1, 1) * w
    return torch.cat([a.sin(), a.cos()], dim=1)


def noising_ref(a, eps, t):
    """float64: x_t = t eps + (1 - t) a (B, D), u = eps - a"""
    a, eps, t = np.asarray(a, np.float64), np.asarray(eps, np.float64), np.asarray(t, np.float64)[:, None]
    return t * eps + (1.0 - t) * a, eps - a


def ulp32(x) -> np.ndarray:
    """the spacing of fp32 at |x| (float64), the subnormal spacing below the normal range"""
    ax = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(ax, np.float32(np.inf)).astype(np.float64) - ax.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ the draw stream
def _philox(group, row, seed: int, offset: int):
    key = ((seed & 0xFFFFFFFF) ^ FLOW_KEY_LO, ((seed >> 32) & 0xFFFFFFFF) ^ FLOW_KEY_HI)
    g, r = np.broadcast_arrays(np.asarray(group, np.uint64), np.asarray(row, np.uint64))
    return philox4x32_10((g, r, np.full(g.shape, offset & 0xFFFFFFFF, np.uint64), np.full(g.shape, (offset >> 32) & 0xFFFFFFFF, np.uint64)), key)


def box_muller_ref(a, b):
    """two uint32 arrays -> (r cos, r sin, r, cos, sin) in float64 from the exact 24-bit uniforms u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24"""
    u1 = ((np.asarray(a, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(b, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return r * np.cos(th), r * np.sin(th), r, np.cos(th), np.sin(th)


def draw_t_uniform(B: int, seed: int, offset: int) -> np.ndarray:
    """(B,) float32, exact: t = (r.x >> 8) 2^-24 of counter (0, row, offset)"""
    r = _philox(np.zeros(B, np.uint64), np.arange(B, dtype=np.uint64), seed, offset)
    return ((r[0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def draw_t_logit_normal(B: int, seed: int, offset: int, a: float, b: float) -> np.ndarray:
    r = _philox(np.zeros(B, np.uint64), np.arange(B, dtype=np.uint64), seed, offset)
    n = box_muller_ref(r[0], r[1])[0]
    return 1.0 / (1.0 + np.exp(-(a + b * n)))


def draw_normals(B: int, D: int, seed: int, offset: int):
    """-> (normals (B, D) float64, bar (B, D) float64): the Box-Muller normals of elements (row, i) and the per-element bound on |fp32 device value - reference|.

    The bound, from the error bounds OpenCL full profile sets for the fp32 functions the ROCm device library implements (log 3 ulp, sqrt 3 ulp, sin / cos
    4 ulp; one ulp is at most 2^-23 relative): r = sqrt(-2 log u1) carries 3 / 2 + 3 ulp; the angle th = fl(2 pi) u2 is off by at most th (2.8e-8 + 2^-24)
    <= 5.5e-7 rad (the rounded constant, one product), which moves cos / sin by as much in absolute terms; cos / sin themselves 4 ulp; the final product half
    an ulp.  |err| <= r (6e-7 + 10 * 2^-23 |trig|)."""
    G = (D + 3) // 4
    rows = np.repeat(np.arange(B, dtype=np.uint64), G)
    groups = np.tile(np.arange(1, G + 1, dtype=np.uint64), B)
    r = _philox(groups, rows, seed, offset)
    out, bar = np.zeros((B * G, 4)), np.zeros((B * G, 4))
    for pair, (a, b) in enumerate(((r[0], r[1]), (r[2], r[3]))):
        nc, ns, rad, c, s = box_muller_ref(a, b)
        out[:, 2 * pair], out[:, 2 * pair + 1] = nc, ns
        bar[:, 2 * pair] = rad * (6e-7 + 10 * 2.0 ** -23 * np.abs(c))
        bar[:, 2 * pair + 1] = rad * (6e-7 + 10 * 2.0 ** -23 * np.abs(s))
    return out.reshape(B, G * 4)[:, :D], bar.reshape(B, G * 4)[:, :D]


# ------------------------------------------------------------------------------------------------------------------ the velocity network
def flow_head_shapes(feat: int, ds: int, da: int, hid: int, fus: int, E: int) -> dict:
    return {"state_projection.0.weight": (ds,), "state_projection.0.bias": (ds,), "state_projection.1.weight": (hid, ds), "state_projection.1.bias": (hid,),
            "fusion.0.weight": (fus, feat + hid + da + E), "fusion.0.bias": (fus,), "fusion.1.weight": (fus,), "fusion.1.bias": (fus,),
            "fusion.4.weight": (fus, fus), "fusion.4.bias": (fus,), "action_head.weight": (da, fus), "action_head.bias": (da,)}


def flow_head_params(shapes: dict, seed: int, scale: float = 0.2) -> dict:
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(*s, generator=g) * (scale if len(s) > 1 else 0.1) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
            for k, s in shapes.items()}


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + LN_EPS) * w + b


def state_branch(p, states):
    return F.silu(F.linear(_ln(states, p["state_projection.0.weight"], p["state_projection.0.bias"]), p["state_projection.1.weight"], p["state_projection.1.bias"]))


def velocity(p: dict, pooled, states, x, phi):
    """the expert with cat = [pooled | s | x | phi]; any dtype (float64 for the reference, float32 for the emulation); autograd works through it"""
    cat = torch.cat([pooled, state_branch(p, states), x, phi], dim=-1)
    f = F.silu(_ln(F.linear(cat, p["fusion.0.weight"], p["fusion.0.bias"]), p["fusion.1.weight"], p["fusion.1.bias"]))
    f = F.silu(F.linear(f, p["fusion.4.weight"], p["fusion.4.bias"]))
    return F.linear(f, p["action_head.weight"], p["action_head.bias"])


def step_times(N: int) -> np.ndarray:
    """(N + 1,) float32: t_i = 1 - i / N rounded once, as the library hands them to its kernels"""
    return (1.0 - np.arange(N + 1, dtype=np.float64) / N).astype(np.float32)


def euler_sample(p: dict, pooled, states, noise, N: int, E: int, *, state_norm=None, action_norm=None, field=None) -> torch.Tensor:
    """float64 Euler sampler.  state_norm = (mean, std, eps) folds the state normalisation in, action_norm = (mean, std) the un-normalisation of the result.
    field(x, t) replaces the network (the linear-Gaussian toy)."""
    p = {k: v.double() for k, v in p.items()}
    pooled, states, x = pooled.double(), states.double(), noise.double().clone()
    if state_norm is not None:
        states = (states - state_norm[0].double()) / (state_norm[1].double() + state_norm[2])
    ts, dt = step_times(N).astype(np.float64), -1.0 / N
    for i in range(N):
        v = field(x, float(ts[i])) if field is not None else velocity(p, pooled, states, x, phi_exact(np.full(x.shape[0], ts[i]), E))
        x = x + dt * v
    if action_norm is not None:
        x = x * action_norm[1].double() + action_norm[0].double()
    return x


def euler_sample_fp32(p: dict, pooled, states, noise, N: int, E: int, *, state_norm=None, action_norm=None) -> torch.Tensor:
    """the same sampler with every operation in fp32 on the CPU (fp32 frequencies, fp32 arguments, fp32 sin / cos, fp32 products and sums): its distance
    from euler_sample is what fp32 arithmetic costs on these inputs, the yardstick of the GPU sampler's bar"""
    p = {k: v.float() for k, v in p.items()}
    pooled, states, x = pooled.float(), states.float(), noise.float().clone()
    if state_norm is not None:
        states = (states - state_norm[0].float()) * (1.0 / (state_norm[1].float() + np.float32(state_norm[2])))
    w = torch.from_numpy(flow_freqs(E))
    ts, dt = step_times(N), np.float32(-1.0 / N)
    for i in range(N):
        a = w * float(ts[i])
        phi = torch.cat([a.sin(), a.cos()]).expand(x.shape[0], -1)
        x = x + float(dt) * velocity(p, pooled, states, x, phi)
    if action_norm is not None:
        x = x * action_norm[1].float() + action_norm[0].float()
    return x


def worst_row_vs_rms(out, ref) -> float:
    """max_b ||out_b - ref_b|| / rms_b ||ref_b||"""
    out, ref = torch.as_tensor(out).double(), torch.as_tensor(ref).double()
    return float((out - ref).norm(dim=1).max() / ref.norm(dim=1).pow(2).mean().sqrt().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------ the sampler cases shared by host and GPU tests
# (feat, ds, hid, fus, K, A, E): the awkward head (fus below the wave size, K A = 21 neither a multiple of 4 nor of 8, E = 6) and the larger one
DIMS = {"awkward": (48, 6, 64, 48, 3, 7, 6), "larger": (96, 14, 128, 192, 50, 14, 64)}
SAMPLER_BATCHES, SAMPLER_STEPS = (1, 9, 67), (1, 4, 10)


def sampler_case(name: str, B: int, seed: int = 0) -> dict:
    """parameters, observation, start noise and dataset statistics of one sampler case.  Weights ~ 1 / sqrt(fan-in) keep every layer's output O(1), so that
    the fp32 emulation stays within 1e-4 of float64 over 10 steps (tests/test_flow_host.py checks exactly that for every case the GPU test runs)."""
    feat, ds, hid, fus, K, A, E = DIMS[name]
    da = K * A
    g = torch.Generator().manual_seed(1000 + seed + 17 * B + (0 if name == "awkward" else 500))
    shapes = flow_head_shapes(feat, ds, da, hid, fus, E)
    p = {k: (torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
         for k, s in shapes.items()}
    return {"dims": DIMS[name], "p": p, "pooled": torch.randn(B, feat, generator=g), "states": torch.randn(B, ds, generator=g) * 2 + 0.5,
            "noise": torch.randn(B, da, generator=g),
            "stats": {"state_mean": torch.randn(ds, generator=g), "state_std": torch.rand(ds, generator=g) + 0.5,
                      "action_mean": torch.randn(da, generator=g), "action_std": torch.rand(da, generator=g) + 0.5}}


def sampler_refs(case: dict, N: int, io: bool):
    """-> (float64 reference, fp32 emulation's distance from it in the sampler's measure)"""
    E, st = case["dims"][6], case["stats"]
    kw = dict(state_norm=(st["state_mean"], st["state_std"], 1e-8), action_norm=(st["action_mean"], st["action_std"])) if io else {}
    ref = euler_sample(case["p"], case["pooled"], case["states"], case["noise"], N, E, **kw)
    emu = euler_sample_fp32(case["p"], case["pooled"], case["states"], case["noise"], N, E, **kw)
    return ref, worst_row_vs_rms(emu, ref)


# ------------------------------------------------------------------------------------------------------------------ the bimodal toy
# the recipe both the GPU test (the project's kernels and AdamW) and the host test (torch) run: dims = (feat, ds, hid, fus, K, A, E)
BIMODAL = {"dims": (32, 4, 32, 64, 1, 2, 16), "batch": 128, "steps": 1500, "lr": 3e-3, "seed": 21}


def bimodal_targets(B: int, D: int, seed: int) -> torch.Tensor:
    """(B, D): +1 in every dimension or -1 in every dimension, exactly half the rows each, in a random order"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.cat([torch.ones(B // 2), -torch.ones(B - B // 2)])[torch.randperm(B, generator=g)]
    return sign.view(B, 1).expand(B, D).contiguous()


def bimodal_observation(B: int, feat: int, ds: int):
    """ONE observation, repeated: the pooled feature and the state are the same in every row"""
    g = torch.Generator().manual_seed(2)
    return torch.randn(1, feat, generator=g).expand(B, -1).contiguous(), torch.randn(1, ds, generator=g).expand(B, -1).contiguous()


def bimodal_init(feat: int, ds: int, da: int, hid: int, fus: int, E, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    shapes = flow_head_shapes(feat, ds, da, hid, fus, E) if E else flow_head_shapes(feat, ds, 0, hid, fus, 0)
    if not E:
        shapes["action_head.weight"], shapes["action_head.bias"] = (da, fus), (da,)
    return {k: (torch.randn(*s, generator=g) / s[-1] ** 0.5 if len(s) > 1 else torch.zeros(*s)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
            for k, s in shapes.items()}


def bimodal_reference(flow: bool) -> dict:
    """the recipe on torch (fp32 parameters, torch.optim.AdamW with the project's betas, no decay, no clipping): mode_stats of 256 samples / predictions"""
    r = BIMODAL
    feat, ds, hid, fus, K, A, E = r["dims"]
    da, B = K * A, r["batch"]
    p = {k: v.clone().requires_grad_(True) for k, v in bimodal_init(feat, ds, da, hid, fus, E if flow else None, r["seed"]).items()}
    opt = torch.optim.AdamW(list(p.values()), lr=r["lr"], betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0)
    targets, (pooled, states) = bimodal_targets(B, da, r["seed"]), bimodal_observation(B, feat, ds)
    g = torch.Generator().manual_seed(r["seed"] + 1)
    w = torch.from_numpy(flow_freqs(E))
    for _ in range(r["steps"]):
        opt.zero_grad()
        if flow:
            eps, t = torch.randn(B, da, generator=g), torch.rand(B, generator=g)
            x = t[:, None] * eps + (1 - t[:, None]) * targets
            a = t[:, None] * w
            loss = ((velocity(p, pooled, states, x, torch.cat([a.sin(), a.cos()], dim=1)) - (eps - targets)) ** 2).mean()
        else:
            cat = torch.cat([pooled, state_branch(p, states)], dim=-1)
            f = F.silu(_ln(F.linear(cat, p["fusion.0.weight"], p["fusion.0.bias"]), p["fusion.1.weight"], p["fusion.1.bias"]))
            f = F.silu(F.linear(f, p["fusion.4.weight"], p["fusion.4.bias"]))
            loss = ((F.linear(f, p["action_head.weight"], p["action_head.bias"]) - targets) ** 2).mean()
        loss.backward()
        opt.step()
    q = {k: v.detach() for k, v in p.items()}
    po, so = pooled[:1].expand(256, -1), states[:1].expand(256, -1)
    if flow:
        out = euler_sample(q, po, so, torch.randn(256, da, generator=g), 10, E)
    else:
        cat = torch.cat([po, state_branch(q, so)], dim=-1)
        f = F.silu(_ln(F.linear(cat, q["fusion.0.weight"], q["fusion.0.bias"]), q["fusion.1.weight"], q["fusion.1.bias"]))
        out = F.linear(F.silu(F.linear(f, q["fusion.4.weight"], q["fusion.4.bias"])), q["action_head.weight"], q["action_head.bias"])
    return mode_stats(out)


def mode_stats(samples) -> dict:
    s = torch.as_tensor(samples).double()
    m = s.mean(dim=1)
    return {"plus": float((m > 0).double().mean()), "minus": float((m < 0).double().mean()), "mean_abs": float(s.abs().mean())}
