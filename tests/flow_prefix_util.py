"""Float64 reference of the flow head's action-prefix conditioning (fv_head_set_flow_prefix; tests only), built on flow_util: the noising with a clean
prefix, the delay draw, the velocity network with the mask block, the prefix Euler sampler with its fp32 CPU emulation (used ONLY to calibrate the GPU
sampler's bar), the cases host and GPU tests share, and the bimodal toy with a pinned first step.

    cat = [ pooled | state branch | x_t | phi(t) | m ],  m[k] = 1 for k < d else 0;  x_t[k] = a[k] (a copy) for k < d
The delay of a head row: word z of the group-0 Philox block whose x and y yield t; d = the smallest j with (z >> 8) < thresholds[j]."""
from __future__ import annotations

import functools

import numpy as np
import torch

import flow_util as fu
import rtc_util as ru

MAX_DELAY = {"awkward": 2, "larger": 12}
SHIFTS = lambda K: (0, 1, K - 1)   # noqa: E731  (K - 1 exercises the K - shift clamp)


# ------------------------------------------------------------------------------------------------------------------ noising and the delay draw
def prefix_noising_ref(a, eps, t, delays, K: int):
    """float64: flow_util.noising_ref with the first delays[r] steps of x_t replaced by a COPY of a; u everywhere as ever"""
    x, u = fu.noising_ref(a, eps, t)
    a = np.asarray(a, np.float64)
    A = a.shape[1] // K
    for r, d in enumerate(np.asarray(delays).astype(int)):
        x[r, :d * A] = a[r, :d * A]
    return x, u


def mask_ref(delays, K: int) -> np.ndarray:
    """(R, K) float64, exact 0.0 / 1.0"""
    return (np.arange(K)[None, :] < np.asarray(delays).astype(int)[:, None]).astype(np.float64)


def draw_delays(B: int, seed: int, offset: int, thresholds) -> np.ndarray:
    """(B,) int64, exact: the smallest j with (z >> 8) < thresholds[j], z = word 2 of counter (0, row, offset)"""
    r = fu._philox(np.zeros(B, np.uint64), np.arange(B, dtype=np.uint64), seed, offset)
    z24 = (np.asarray(r[2], np.uint32) >> np.uint32(8)).astype(np.int64)
    return np.searchsorted(np.asarray(thresholds, dtype=np.int64), z24, side="right")


# ------------------------------------------------------------------------------------------------------------------ the network with the mask block
def prefix_head_shapes(feat: int, ds: int, da: int, hid: int, fus: int, E: int, K: int) -> dict:
    s = fu.flow_head_shapes(feat, ds, da, hid, fus, E)
    s["fusion.0.weight"] = (fus, feat + hid + da + E + K)
    return s


def velocity(p: dict, pooled, states, x, phi, m):
    """flow_util.velocity with cat = [pooled | s | x | phi | m] (it concatenates what it is handed)"""
    return fu.velocity(p, pooled, states, x, torch.cat([phi, m.to(phi.dtype)], dim=-1))


def drop_mask_columns(p: dict, K: int) -> dict:
    q = dict(p)
    q["fusion.0.weight"] = p["fusion.0.weight"][:, :-K].contiguous()
    return q


# ------------------------------------------------------------------------------------------------------------------ the prefix sampler
def pinned_steps(delays, D: int, K: int, shift: int) -> np.ndarray:
    return np.minimum(np.minimum(np.maximum(np.asarray(delays).astype(int), 0), D), K - shift)


def prefix_euler_sample(p: dict, pooled, states, noise, prev, delays, shift: int, N: int, E: int, K: int, D: int, *, state_norm=None, action_norm=None,
                        fp32: bool = False):
    """-> (actions, chunk).  Row b's first p_b = min(delays[b], D, K - shift) steps start as prev[b][k + shift] and are never updated; the mask block reads
    m[k] = [k < p_b].  fp32 = True: every operation in fp32 on the CPU (flow_util.euler_sample_fp32's recipe), the emulation."""
    dt_ = torch.float32 if fp32 else torch.float64
    p = {k: v.to(dt_) for k, v in p.items()}
    B, da = noise.shape
    A = da // K
    pin = pinned_steps(delays, D, K, shift)
    m = torch.from_numpy(mask_ref(pin, K)).to(dt_)
    live = ~(m.bool().repeat_interleave(A, dim=1))
    x = noise.to(dt_).clone()
    pv = torch.as_tensor(prev).to(dt_)
    for b in range(B):
        n = int(pin[b]) * A
        x[b, :n] = pv[b, shift * A:shift * A + n]
    pooled, states = pooled.to(dt_), states.to(dt_)
    if state_norm is not None:
        if fp32:
            states = (states - state_norm[0].float()) * (1.0 / (state_norm[1].float() + np.float32(state_norm[2])))
        else:
            states = (states - state_norm[0].double()) / (state_norm[1].double() + state_norm[2])
    ts = fu.step_times(N)
    dt = float(np.float32(-1.0 / N)) if fp32 else -1.0 / N
    wfreq = torch.from_numpy(fu.flow_freqs(E))
    for i in range(N):
        if fp32:
            a = wfreq * float(ts[i])
            phi = torch.cat([a.sin(), a.cos()]).expand(B, -1)
        else:
            phi = fu.phi_exact(np.full(B, ts[i]), E)
        v = velocity(p, pooled, states, x, phi, m)
        x = torch.where(live, x + dt * v, x)
    chunk = x
    if action_norm is not None:
        x = x * action_norm[1].to(dt_) + action_norm[0].to(dt_)
    return x, chunk


# ------------------------------------------------------------------------------------------------------------------ shared cases
def case_delays(B: int, D: int) -> np.ndarray:
    """mixed over 0 .. D, one row above D (clamped) once B > D + 1; row 0 pins D steps"""
    return ((D - np.arange(B)) % (D + 2)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def prefix_case(name: str, B: int) -> dict:
    """rtc_util.rtc_case (parameters, observation, start noise, statistics, a plausible previous chunk) with K mask columns ~ 1 / sqrt(fan-in) behind
    fusion.0.weight, and the rows' delays.  Cached: computed once per session and left unchanged."""
    case = dict(ru.rtc_case(name, B))
    K, D = case["dims"][4], MAX_DELAY[name]
    g = torch.Generator().manual_seed(777 + B)
    p = dict(case["p"])
    w = p["fusion.0.weight"]
    p["fusion.0.weight"] = torch.cat([w, torch.randn(w.shape[0], K, generator=g) / (w.shape[1] + K) ** 0.5], dim=1)
    case["p"], case["D"], case["delays"] = p, D, case_delays(B, D)
    return case


@functools.lru_cache(maxsize=None)
def prefix_refs(name: str, B: int, N: int, io: bool, shift: int):
    """-> (actions64, chunk64, emulation distance of actions, of chunk) for one GPU sampler case"""
    c = prefix_case(name, B)
    K, E = c["dims"][4], c["dims"][6]
    args = (c["p"], c["pooled"], c["states"], c["noise"], c["prev"], c["delays"], shift, N, E, K, c["D"])
    act, chunk = prefix_euler_sample(*args, **ru.io_kwargs(c, io))
    act32, chunk32 = prefix_euler_sample(*args, **ru.io_kwargs(c, io), fp32=True)
    return act, chunk, fu.worst_row_vs_rms(act32, act), fu.worst_row_vs_rms(chunk32, chunk)


# ------------------------------------------------------------------------------------------------------------------ one head step
def step_reference(p: dict, pooled, states, a, eps, t, delays, pad, kind: str, dims, dim_w=None, step_w=None) -> dict:
    """float64 autograd of prepare, forward, loss, backward: a conditioned step is masked like a padded one; the divisor stays all R K A elements.
    a (B, da) per observation; eps, t, delays per head row (R = S B rows, draw-major); pad (B, K) bool numpy or None"""
    import flow_draws_util as du
    feat, ds, hid, fus, K, A, E = dims
    B, R = a.shape[0], eps.shape[0]
    n = R // B
    p64 = {k: w.detach().double().requires_grad_(True) for k, w in p.items()}
    x_ref, u_ref = prefix_noising_ref(np.tile(a.numpy(), (n, 1)), eps.numpy(), t.numpy(), delays, K)
    m = mask_ref(delays, K)
    phi = fu.phi_ref(t.numpy(), fu.flow_freqs(E))
    pred = velocity(p64, pooled.double().repeat(n, 1), states.double().repeat(n, 1), torch.from_numpy(x_ref), torch.from_numpy(phi), torch.from_numpy(m))
    masked = m.astype(bool) | (np.tile(np.asarray(pad, dtype=bool), (n, 1)) if pad is not None else False)
    loss = du.loss_ref(pred.view(R, K, A), torch.from_numpy(u_ref).view(R, K, A), torch.from_numpy(masked), kind, dim_w, step_w)
    loss.backward()
    return {"loss": loss.detach(), "pred": pred.detach(), "grads": {k: w.grad for k, w in p64.items()}}


# ------------------------------------------------------------------------------------------------------------------ the bimodal toy with a pinned first step
# flow_util.BIMODAL's recipe (same optimiser, batch, step count, learning rate and seed) on a chunk of K = 4 steps of A = 1 dimension, D = 2: every target chunk
# lies wholly in the + mode or wholly in the - mode, so a sampler that honours a pinned + first step must put the other three steps in the + mode
PREFIX_BIMODAL = {"dims": (32, 4, 32, 64, 4, 1, 16), "D": 2, "batch": 128, "steps": 1500, "lr": 3e-3, "seed": 21, "samples": 512}


def prefix_bimodal_init(seed: int) -> dict:
    feat, ds, hid, fus, K, A, E = PREFIX_BIMODAL["dims"]
    p = fu.bimodal_init(feat, ds, K * A, hid, fus, E, seed)
    g = torch.Generator().manual_seed(seed + 100)
    w = p["fusion.0.weight"]
    p["fusion.0.weight"] = torch.cat([w, torch.randn(w.shape[0], K, generator=g) / (w.shape[1] + K) ** 0.5], dim=1)
    return p


def pinned_stats(chunk) -> dict:
    """chunk (n, 4): the fraction of rows whose steps 1 .. 3 land in the + mode (their mean is positive)"""
    rest = torch.as_tensor(chunk).double()[:, 1:]
    return {"plus": float((rest.mean(dim=1) > 0).double().mean()), "mean_abs": float(rest.abs().mean())}


def prefix_bimodal_reference() -> dict:
    """the recipe on torch (fp32 parameters, torch.optim.AdamW with the project's betas): delays uniform over 0 .. D per row, conditioned steps out of the
    loss, the divisor all B K A elements.  -> {"pinned": pinned_stats of 512 samples whose first step is pinned to +1, "free": mode_stats of 512 unpinned}"""
    r = PREFIX_BIMODAL
    feat, ds, hid, fus, K, A, E = r["dims"]
    da, B, D, n = K * A, r["batch"], r["D"], r["samples"]
    p = {k: v.clone().requires_grad_(True) for k, v in prefix_bimodal_init(r["seed"]).items()}
    opt = torch.optim.AdamW(list(p.values()), lr=r["lr"], betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0)
    targets, (pooled, states) = fu.bimodal_targets(B, da, r["seed"]), fu.bimodal_observation(B, feat, ds)
    g = torch.Generator().manual_seed(r["seed"] + 1)
    w = torch.from_numpy(fu.flow_freqs(E))
    for _ in range(r["steps"]):
        opt.zero_grad()
        eps, t = torch.randn(B, da, generator=g), torch.rand(B, generator=g)
        d = torch.randint(0, D + 1, (B,), generator=g)
        m = (torch.arange(K)[None, :] < d[:, None]).float()
        me = m.repeat_interleave(A, dim=1)
        x = torch.where(me.bool(), targets, t[:, None] * eps + (1 - t[:, None]) * targets)
        a = t[:, None] * w
        pred = velocity(p, pooled, states, x, torch.cat([a.sin(), a.cos()], dim=1), m)
        loss = (((pred - (eps - targets)) ** 2) * (1 - me)).sum() / me.numel()
        loss.backward()
        opt.step()
    q = {k: v.detach() for k, v in p.items()}
    po, so = pooled[:1].expand(n, -1), states[:1].expand(n, -1)
    prev = torch.ones(n, da)
    _, pinned = prefix_euler_sample(q, po, so, torch.randn(n, da, generator=g), prev, np.ones(n, dtype=np.int32), 0, 10, E, K, D)
    _, free = prefix_euler_sample(q, po, so, torch.randn(n, da, generator=g), prev, np.zeros(n, dtype=np.int32), 0, 10, E, K, D)
    return {"pinned": pinned_stats(pinned), "free": fu.mode_stats(free)}


# ------------------------------------------------------------------------------------------------------------------ pieces the GPU tests share
# (kept here, not imported from other test modules: a test file is no library)
def saved_cat(eng, saved, B: int):
    """the (draws * B, cat width) view of fusion.0's input `cat` inside `saved`, at the offset the library itself reports (fv_op_head_saved_cat_offset)"""
    import ctypes as C
    from fastvla_hip import _lib
    hd, S, cw = eng.head_dims, eng.head_flow_draws, eng.head_cat_width()
    E = eng.head_flow["time_dim"] if eng.head_flow else 0
    pk = eng.head_flow_prefix["chunk"] if eng.head_flow_prefix else 0
    off = C.c_size_t()
    _lib.check(_lib.load_testops().fv_op_head_saved_cat_offset(hd["feat"], hd["ds"], hd["da"], hd["hid"], hd["fus"], E, S, pk, B, C.byref(off)), "fv_op_head_saved_cat_offset")
    return saved[off.value:off.value + S * B * cw].view(S * B, cw)


# the backbone-route rig: test_gpu_flow_draws' shapes for the same comparison (synthetic "small" model), and the bar its route comparison uses
ROUTE = dict(B=3, T=16, K=4, A=5, hd=64, E=6, rank=16, seed=1234, offset=(2 << 44) + (40 << 16) + 1)
ROUTE_GRAD_TOL = 2e-3


def route_inputs(model, B: int, T: int, seed: int):
    """tower output, token ids (one repeated inside a row and across rows), a ragged attention mask, states"""
    g = torch.Generator().manual_seed(seed)
    tower_out = (torch.randn(B, model.tower.num_tokens, model.tower.out_dim, generator=g) * 0.7).to(torch.bfloat16)
    ids = torch.randint(0, model.llm.vocab, (B, T), generator=g)
    ids[0, 3] = ids[0, 1]
    ids[1, 0] = ids[0, 1]
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, T // 2 + 1:] = 0
    if B > 2:
        mask[2, 1:] = 0
    return tower_out, ids, mask, torch.randn(B, 14, generator=g)


def random_adapters(lflat, ltensors, seed: int, b_std: float = 0.05) -> None:
    """LoRA adapters with a non-zero B (the default initialisation leaves the adapted model equal to the base model)"""
    from fastvla_hip import lora
    lora.init_adapters(lflat, ltensors, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    for name, v in lora.adapter_views(lflat, ltensors).items():
        if name.endswith(".lora_B.weight"):
            v.copy_((torch.randn(v.shape, generator=g) * b_std).to(v.device))


def policy_batch(B: int, K: int, seed: int, device=None) -> dict:
    """a training batch of the tiny policy: row 0 has its last step padded"""
    g = torch.Generator().manual_seed(seed)
    pad = torch.zeros(B, K, dtype=torch.bool)
    pad[0, K - 1:] = True
    batch = {"images": torch.rand(B, 3, 72, 96, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, K, 14, generator=g),
             "action_is_pad": pad, "tasks": ["stack the red block", "open drawer", "x", "push"][:B]}
    return batch if device is None else {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
