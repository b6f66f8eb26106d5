"""Real-time chunking for the flow head (Black, Galliker, Levine 2025; fv_head_set_flow_guidance / fv_head_flow_sample_guided): the new chunk is sampled
guided by the not-yet-executed rest of the previous one.

`prefix_weights` is the host-side definition of the per-step weights the library uploads: for a chunk of K steps, an inference delay d (the steps that will be
executed while inference runs: a hard prefix of weight 1) and an execution horizon s (the last s steps are left free),
    "exp"    w[k] = 1 (k < d),  c (e^c - 1) / (e - 1) with c = (K - s - k) / (K - s - d + 1)  (d <= k < K - s),  0 (k >= K - s)      -- the paper's
    "linear" w[k] = c on the middle range
    "ones"   1 on the whole overlap k < K - s
    "zeros"  1 on k < d only
(the four names are LeRobot's).  `guidance_weight` is the per-step factor k_i the sampler applies.  `RealTimeChunker` owns, per engine, the device buffer that
holds the previous chunk of n_env environments and the row mask that says which of them have one."""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

SCHEDULES = ("exp", "linear", "ones", "zeros")


def check_rtc(K, inference_delay, execution_horizon, schedule="exp") -> Tuple[int, int, int]:
    """-> (K, d, s) as ints; ValueError unless K >= 1, 0 <= d, 1 <= s, d + s <= K and the schedule is known"""
    if schedule not in SCHEDULES:
        raise ValueError(f"rtc_schedule must be one of {SCHEDULES}, got {schedule!r}")
    for name, v, lo in (("chunk_size", K, 1), ("inference_delay", inference_delay, 0), ("execution_horizon", execution_horizon, 1)):
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    if inference_delay + execution_horizon > K:
        raise ValueError(f"inference_delay + execution_horizon must not exceed chunk_size: {inference_delay} + {execution_horizon} > {K}")
    return int(K), int(inference_delay), int(execution_horizon)


def prefix_weights(K: int, inference_delay: int, execution_horizon: int, schedule: str = "exp") -> List[float]:
    """-> K python floats in double (the library rounds them to fp32 once)"""
    K, d, s = check_rtc(K, inference_delay, execution_horizon, schedule)
    w = []
    for k in range(K):
        if k < d:
            w.append(1.0)
        elif k >= K - s:
            w.append(0.0)
        elif schedule == "ones":
            w.append(1.0)
        elif schedule == "zeros":
            w.append(0.0)
        else:
            c = (K - s - k) / (K - s - d + 1)
            w.append(c if schedule == "linear" else c * math.expm1(c) / (math.e - 1.0))
    return w


def guidance_weight(t: float, beta: float) -> float:
    """k_i of the Euler step at time t (t = 1 is noise): beta at t = 1, else min(beta, ((1 - t)^2 + t^2) / ((1 - t) t)), in double"""
    t = float(t)
    if not 0.0 < t <= 1.0:
        raise ValueError(f"t must lie in (0, 1], got {t}")
    return float(beta) if t == 1.0 else min(float(beta), ((1.0 - t) ** 2 + t * t) / ((1.0 - t) * t))


class RealTimeChunker:
    """The previous chunk of n_env environments on the engine's device: `prev` (n_env, da) f32 in normalised space and `has_prev` (n_env) int32, the row mask
    of the guided sampler.  sample() runs one guided call over all rows and keeps the new chunk; reset(env=None) clears the mask (stream-ordered, no host
    synchronisation), so the next plan of those rows is unguided."""

    def __init__(self, engine, n_env: int):
        if isinstance(n_env, bool) or int(n_env) != n_env or int(n_env) < 1:
            raise ValueError(f"RealTimeChunker: n_env must be an integer >= 1, got {n_env!r}")
        self._engine, self.n_env = engine, int(n_env)
        da = engine.head_dims["da"]
        with torch.inference_mode(False):      # (created from inside select_action's inference mode, reset from outside it: ordinary tensors)
            self.prev = torch.zeros(self.n_env, da, dtype=torch.float32, device=engine.device)
            self.has_prev = torch.zeros(self.n_env, dtype=torch.int32, device=engine.device)
            self._next = torch.empty_like(self.prev)

    def reset(self, env: Optional[int] = None) -> None:
        if env is None:
            self.has_prev.zero_()
            return
        if isinstance(env, bool) or int(env) != env or not 0 <= int(env) < self.n_env:
            raise ValueError(f"env must be None or in 0 .. {self.n_env - 1}, got {env!r}")
        self.has_prev[int(env)].zero_()

    def sample(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, *, shift: int, steps: int, noise: Optional[torch.Tensor] = None,
               seed: int = 0, offset: int = 0, prev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> actions (n_env, da).  prev: an explicit previous chunk for every row (normalised; all rows are then guided); None: the kept one under has_prev"""
        if pooled.shape[0] != self.n_env:
            raise ValueError(f"this chunker holds {self.n_env} environments, the batch has {pooled.shape[0]}")
        explicit = prev is not None
        actions, _ = self._engine.head_flow_sample_guided(flat_params, pooled, states, prev if explicit else self.prev, shift=shift,
                                                          row_mask=None if explicit else self.has_prev, steps=steps, noise=noise, seed=seed, offset=offset,
                                                          chunk_out=self._next)
        self.prev, self._next = self._next, self.prev
        self.has_prev.fill_(1)
        return actions

    def sample_prefix(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, *, shift: int, delay: int, steps: int,
                      noise: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0, prev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> actions (n_env, da): the prefix sampler (fv_head_flow_sample_prefix; a head trained with set_head_flow_prefix) in place of the guided one.  Every
        row pins its first min(delay, max_delay, K - shift) steps to the kept chunk read `shift` steps ahead; the row mask becomes per-row delays, so a
        row without a previous chunk has delay 0 and pins nothing.  prev: an explicit previous chunk for every row, as in sample()"""
        if pooled.shape[0] != self.n_env:
            raise ValueError(f"this chunker holds {self.n_env} environments, the batch has {pooled.shape[0]}")
        explicit = prev is not None
        delays = torch.full_like(self.has_prev, int(delay)) if explicit else self.has_prev * int(delay)      # (device arithmetic: no host synchronisation)
        actions, _ = self._engine.head_flow_sample_prefix(flat_params, pooled, states, prev if explicit else self.prev, delays, shift=shift, steps=steps,
                                                          noise=noise, seed=seed, offset=offset, chunk_out=self._next)
        self.prev, self._next = self._next, self.prev
        self.has_prev.fill_(1)
        return actions

    def sample_multi(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, *, samples: int, select: str, shift: int, steps: int,
                     delay: Optional[int] = None, noise: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0, prev: Optional[torch.Tensor] = None) -> dict:
        """-> head_flow_sample_multi's dict: `samples` candidates per row in one call, one of them chosen (fv_head_flow_sample_multi), and the CHOSEN chunk
        kept as the next call's previous one.  select "coherent" scores every candidate against the kept chunk read `shift` steps ahead; a row without one
        (has_prev 0) takes the medoid.  delay (None: the plain sampler): the candidates come from the prefix sampler, as in sample_prefix()"""
        if pooled.shape[0] != self.n_env:
            raise ValueError(f"this chunker holds {self.n_env} environments, the batch has {pooled.shape[0]}")
        explicit = prev is not None
        delays = None if delay is None else (torch.full_like(self.has_prev, int(delay)) if explicit else self.has_prev * int(delay))
        out = self._engine.head_flow_sample_multi(flat_params, pooled, states, samples=samples, select=select, prev=prev if explicit else self.prev, shift=shift,
                                                  row_mask=None if explicit else self.has_prev, delays=delays, steps=steps, noise=noise, seed=seed, offset=offset,
                                                  chunk_out=self._next)
        self.prev, self._next = self._next, self.prev
        self.has_prev.fill_(1)
        return out
