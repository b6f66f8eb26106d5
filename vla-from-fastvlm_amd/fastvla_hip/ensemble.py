"""Temporal ensembling of action chunks on the device (fv_ensemble_*; ACT's exponential weighting as LeRobot's ACTTemporalEnsembler does it, per environment).

Every control step the policy predicts K future steps; the action served for time t is the weighted mean of what the chunks predicted at t-K+1 .. t say
about t, with weights exp(-coeff i), i = 0 the OLDEST prediction (coeff 0: uniform; negative: newer predictions count more).  The running means live in a
device ring of (n_env, K, A) floats; step() is one kernel launch and never synchronises the host, so a batch of environments is ensembled inside the loop.
`reference_weights` is the host-side definition of the two tables the library uploads."""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import Optional

import torch

from . import _lib


def check_coeff(coeff) -> float:
    """-> coeff as a float; ValueError unless it is a finite number"""
    try:
        c = float(coeff)
    except (TypeError, ValueError):
        raise ValueError(f"temporal_ensemble_coeff must be a finite number, got {coeff!r}") from None
    if not math.isfinite(c):
        raise ValueError(f"temporal_ensemble_coeff must be a finite number, got {coeff!r}")
    return c


def reference_weights(coeff: float, chunk: int):
    """-> (w, cumsum_w): K python floats each, w[i] = exp(-coeff i) and its running sum, in double (the library rounds both to fp32 once)"""
    w = [math.exp(-float(coeff) * i) for i in range(int(chunk))]
    cw, run = [], 0.0
    for x in w:
        run += x
        cw.append(run)
    return w, cw


class TemporalEnsembler:
    """Owner of one fv_ensembler: step(chunks (n_env, K, A)) -> (n_env, A), reset(env=None).  The ring position is host state of the library object, so
    step() must not run inside a captured graph."""

    def __init__(self, engine, n_env: int, chunk: int, step_dim: int, coeff: float):
        coeff = check_coeff(coeff)
        for name, v in (("n_env", n_env), ("chunk", chunk), ("step_dim", step_dim)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"TemporalEnsembler: {name} must be an integer >= 1, got {v}")
        self._engine, self.n_env, self.chunk, self.step_dim, self.coeff = engine, int(n_env), int(chunk), int(step_dim), coeff
        out = C.c_void_p()
        with torch.cuda.device(engine.device):
            _lib.check(engine.lib.fv_ensemble_create(engine.h, self.n_env, self.chunk, self.step_dim, coeff, C.byref(out)), "fv_ensemble_create", engine.h)
        self._h = out.value
        engine.__dict__.setdefault("_group_tables", weakref.WeakSet()).add(self)      # (closed before the engine's handle, as the parameter-group tables are)

    def handle(self) -> int:
        if not self._h:
            raise _lib.FastVLAHipError("this temporal ensembler has been closed")
        return self._h

    def step(self, chunks: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """chunks: (n_env, K, A) (or (n_env, K * A)) f32 on the engine's device, the chunks predicted at this time step -> the ensembled actions (n_env, A)"""
        eng = self._engine
        if chunks.numel() != self.n_env * self.chunk * self.step_dim or chunks.shape[0] != self.n_env:
            raise ValueError(f"chunks must be ({self.n_env}, {self.chunk}, {self.step_dim}), got {tuple(chunks.shape)}")
        chunks = chunks.to(device=eng.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty(self.n_env, self.step_dim, dtype=torch.float32, device=eng.device)
        elif out.shape != (self.n_env, self.step_dim) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != eng.device:
            raise ValueError(f"out must be a contiguous f32 ({self.n_env}, {self.step_dim}) tensor on {eng.device}")
        _lib.check(eng.lib.fv_ensemble_step(eng.h, self.handle(), chunks.data_ptr(), out.data_ptr(), torch.cuda.current_stream(eng.device).cuda_stream),
                   "fv_ensemble_step", eng.h)
        return out

    def reset(self, env: Optional[int] = None) -> None:
        """forget the history of one environment, or of all (None); stream-ordered, no host synchronisation"""
        eng = self._engine
        e = -1 if env is None else int(env)
        if e < -1 or e >= self.n_env or (env is not None and e < 0):
            raise ValueError(f"env must be None or in 0 .. {self.n_env - 1}, got {env}")
        _lib.check(eng.lib.fv_ensemble_reset(eng.h, self.handle(), e, torch.cuda.current_stream(eng.device).cuda_stream), "fv_ensemble_reset", eng.h)

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self._engine, "h", None):      # (after the engine's fv_destroy only the host record is left: dropped with this object)
            _lib.check(self._engine.lib.fv_ensemble_destroy(self._engine.h, h), "fv_ensemble_destroy", self._engine.h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
