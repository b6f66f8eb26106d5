"""The guarded optimiser step (include/fastvla_hip.h fv_step_guard): skip a step whose gradient is non-finite or came from saturated fp16 operands, and keep a
dynamic loss scale, all on the device -- what torch.cuda.amp.GradScaler does around an optimiser, without its host read.

Options (what policy.enable_step_guard takes; each has an environment twin an explicit argument beats, FASTVLA_STEP_GUARD=1 alone switches the guard on):
  dynamic_loss_scale   True: delta = 2^delta_log2 on top of the static loss scale 2^k moves inside the bounds below;      FASTVLA_STEP_GUARD_DYNAMIC_LOSS_SCALE
                       False: delta is pinned at 1 and the guard only skips
  growth_interval      applied steps without a skip after which delta grows (GradScaler's 2000)                           FASTVLA_STEP_GUARD_GROWTH_INTERVAL
  backoff_log2         delta's exponent goes down by this on a skipped step (1: halve)                                     FASTVLA_STEP_GUARD_BACKOFF_LOG2
  growth_log2          ... and up by this after growth_interval good steps (1: double)                                     FASTVLA_STEP_GUARD_GROWTH_LOG2
  min_loss_scale_log2  bounds of the WHOLE scale's exponent k + delta_log2, inside fv_train_set_options' [0, 24]           FASTVLA_STEP_GUARD_MIN_LOSS_SCALE_LOG2
  max_loss_scale_log2                                                                                                      FASTVLA_STEP_GUARD_MAX_LOSS_SCALE_LOG2
`StepGuard` owns one fv_step_guard; `guard_config` turns the options and a static exponent k into its delta range."""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Dict, Optional

from . import _lib

OPTION_KEYS = ("dynamic_loss_scale", "growth_interval", "backoff_log2", "growth_log2", "min_loss_scale_log2", "max_loss_scale_log2")
DEFAULTS = {"dynamic_loss_scale": True, "growth_interval": 2000, "backoff_log2": 1, "growth_log2": 1, "min_loss_scale_log2": 0, "max_loss_scale_log2": 24}
STATE_KEYS = ("delta_log2", "good_steps", "last_apply", "last_inv_delta", "flag", "last_saturations", "applied", "skipped_nonfinite", "skipped_saturated",
              "saturated_applied")
LOSS_SCALE_LOG2_RANGE = (0, 24)      # fv_train_set_options' bounds
_TRUE, _FALSE = ("1", "true", "yes", "on"), ("0", "false", "no", "off")
_ENV = "FASTVLA_STEP_GUARD"


def _int(name: str, value, lo: int, hi: Optional[int] = None) -> int:
    try:
        v = int(value)
        if isinstance(value, bool) or v != float(value):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"step guard {name} must be an integer, got {value!r}") from None
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"step guard {name} must be {'in [' + str(lo) + ', ' + str(hi) + ']' if hi is not None else '>= ' + str(lo)}, got {value!r}")
    return v


def normalize_options(dynamic_loss_scale=True, growth_interval=2000, backoff_log2=1, growth_log2=1, min_loss_scale_log2=0, max_loss_scale_log2=24) -> Dict:
    """-> the six options, checked.  ValueError: a dynamic_loss_scale that is no boolean, a growth_interval < 1, a negative or fractional exponent step, bounds
    outside [0, 24], or min_loss_scale_log2 above max_loss_scale_log2 (the message names both)."""
    if not isinstance(dynamic_loss_scale, (bool, int)) or dynamic_loss_scale not in (0, 1):
        raise ValueError(f"step guard dynamic_loss_scale must be a boolean, got {dynamic_loss_scale!r}")
    lo, hi = LOSS_SCALE_LOG2_RANGE
    out = {"dynamic_loss_scale": bool(dynamic_loss_scale), "growth_interval": _int("growth_interval", growth_interval, 1, 2 ** 31 - 1),
           "backoff_log2": _int("backoff_log2", backoff_log2, 0, 48), "growth_log2": _int("growth_log2", growth_log2, 0, 48),
           "min_loss_scale_log2": _int("min_loss_scale_log2", min_loss_scale_log2, lo, hi),
           "max_loss_scale_log2": _int("max_loss_scale_log2", max_loss_scale_log2, lo, hi)}
    if out["min_loss_scale_log2"] > out["max_loss_scale_log2"]:
        raise ValueError(f"step guard min_loss_scale_log2={out['min_loss_scale_log2']} is above max_loss_scale_log2={out['max_loss_scale_log2']}")
    return out


def _env_values(environ=None) -> Dict:
    """the twins that are set, as strings / booleans (unset and empty are the same)"""
    env = os.environ if environ is None else environ
    kw: Dict = {}
    for k in OPTION_KEYS:
        raw = (env.get(f"{_ENV}_{k.upper()}") or "").strip()
        if not raw:
            continue
        if k == "dynamic_loss_scale":
            if raw.lower() not in _TRUE + _FALSE:
                raise ValueError(f"{_ENV}_{k.upper()} must be one of {', '.join(_TRUE + _FALSE)}, got '{raw}'")
            kw[k] = raw.lower() in _TRUE
        else:
            try:
                kw[k] = int(raw)
            except ValueError:
                raise ValueError(f"{_ENV}_{k.upper()} must be an integer, got '{raw}'") from None
    return kw


def enabled_from_env(environ=None) -> bool:
    env = os.environ if environ is None else environ
    raw = (env.get(_ENV) or "").strip().lower()
    if raw and raw not in _TRUE + _FALSE:
        raise ValueError(f"{_ENV} must be one of {', '.join(_TRUE + _FALSE)}, got '{raw}'")
    return raw in _TRUE


def options_from_env(environ=None) -> Optional[Dict]:
    """FASTVLA_STEP_GUARD=1 (with its FASTVLA_STEP_GUARD_* twins) -> normalize_options' dict; None when it is not set: the twins alone switch nothing on.
    Malformed values raise ValueError."""
    return normalize_options(**_env_values(environ)) if enabled_from_env(environ) else None


def resolve_options(environ=None, **given) -> Dict:
    """what enable_step_guard(...) runs with: per option the explicit argument (not None), else its environment twin, else the default"""
    unknown = set(given) - set(OPTION_KEYS)
    if unknown:
        raise TypeError(f"unknown step guard options {sorted(unknown)}")
    kw = _env_values(environ)
    kw.update({k: v for k, v in given.items() if v is not None})
    return normalize_options(**kw)


def guard_config(options: Dict, loss_scale_log2: Optional[int]) -> Dict:
    """-> StepGuard's keywords for a run whose static loss scale is 2^loss_scale_log2 (None: head-only training, fp32 without a loss scale).  delta starts at 1;
    its exponent may move in [min_loss_scale_log2 - k, max_loss_scale_log2 - k].  dynamic_loss_scale=False, or no loss scale at all, pins delta = 1.
    ValueError, naming both settings, when k lies outside the bounds."""
    o = normalize_options(**dict(options))
    cfg = {"init_delta_log2": 0, "min_delta_log2": 0, "max_delta_log2": 0, "growth_interval": o["growth_interval"], "backoff_log2": o["backoff_log2"],
           "growth_log2": o["growth_log2"], "skip_on_saturation": True}
    if loss_scale_log2 is not None and o["dynamic_loss_scale"]:
        k = int(loss_scale_log2)
        if not o["min_loss_scale_log2"] <= k <= o["max_loss_scale_log2"]:
            raise ValueError(f"the loss scale 2^{k} (train_set_options loss_scale_log2={k}) lies outside the step guard's bounds min_loss_scale_log2="
                             f"{o['min_loss_scale_log2']}, max_loss_scale_log2={o['max_loss_scale_log2']}")
        cfg["min_delta_log2"], cfg["max_delta_log2"] = o["min_loss_scale_log2"] - k, o["max_loss_scale_log2"] - k
    return cfg


def all_reduce_flag(flag, group=None) -> None:
    """the data-parallel exchange of the guard's flag: SUM over the ranks, in place on the one-float tensor, so that every rank decides the same (any value
    > 0 counts as set).  A single process, or torch.distributed not initialised: nothing is called."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    dist.all_reduce(flag, op=dist.ReduceOp.SUM, group=group)


class _DevFloat:
    """one float of device memory the library owns, as the CUDA array interface describes it (torch.as_tensor aliases it, no copy)"""

    def __init__(self, ptr: int):
        self.__cuda_array_interface__ = {"shape": (1,), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}


class StepGuard:
    """Owner of one fv_step_guard.  engine.adamw_step(..., guard=) takes it on all four paths; engine.train_set_step_guard(guard) binds it to the training
    backward.  observe() / the step are stream-ordered and read nothing back; state() and load_state() synchronise (status calls)."""

    def __init__(self, engine, init_delta_log2: int = 0, min_delta_log2: int = 0, max_delta_log2: int = 0, growth_interval: int = 2000, backoff_log2: int = 1,
                 growth_log2: int = 1, skip_on_saturation: bool = True):
        import torch
        self._engine = engine
        self.config = dict(init_delta_log2=int(init_delta_log2), min_delta_log2=int(min_delta_log2), max_delta_log2=int(max_delta_log2),
                           growth_interval=int(growth_interval), backoff_log2=int(backoff_log2), growth_log2=int(growth_log2),
                           skip_on_saturation=bool(skip_on_saturation))
        c = self.config
        cfg = _lib.StepGuardConfig(c["init_delta_log2"], c["min_delta_log2"], c["max_delta_log2"], c["growth_interval"], c["backoff_log2"], c["growth_log2"],
                                   int(c["skip_on_saturation"]), 0)
        out = C.c_void_p()
        with torch.cuda.device(engine.device):
            _lib.check(engine.lib.fv_step_guard_create(engine.h, C.byref(cfg), C.byref(out)), "fv_step_guard_create", engine.h)
        self._h = out.value
        self._flag = None
        engine.__dict__.setdefault("_group_tables", weakref.WeakSet()).add(self)      # (closed before the engine's handle, as the parameter-group tables are)

    def handle(self) -> int:
        if not self._h:
            raise _lib.FastVLAHipError("this step guard has been closed")
        return self._h

    def observe(self) -> None:
        """after a backward, on the current stream: the flag is set if the engine's fp16 saturation counter moved since the last look"""
        import torch
        eng = self._engine
        _lib.check(eng.lib.fv_step_guard_observe(eng.h, self.handle(), torch.cuda.current_stream(eng.device).cuda_stream), "fv_step_guard_observe", eng.h)

    def flag(self):
        """-> the (1,) f32 device tensor that IS the guard's sticky flag (no copy): what all_reduce_flag sums across ranks before the step"""
        import torch
        if self._flag is None:
            eng, p = self._engine, C.c_void_p()
            _lib.check(eng.lib.fv_step_guard_flag(eng.h, self.handle(), C.byref(p)), "fv_step_guard_flag", eng.h)
            with torch.cuda.device(eng.device):
                self._flag = torch.as_tensor(_DevFloat(p.value), device=eng.device)
        return self._flag

    def report(self):
        """-> (2,) f32 device tensor { 1 if the last guarded step was skipped else 0, the delta the next backward runs with }: one small launch, no host read"""
        import torch
        eng = self._engine
        out = torch.empty(2, dtype=torch.float32, device=eng.device)
        _lib.check(eng.lib.fv_step_guard_report(eng.h, self.handle(), out.data_ptr(), torch.cuda.current_stream(eng.device).cuda_stream), "fv_step_guard_report",
                   eng.h)
        return out

    def state(self) -> Dict:
        """fv_step_guard_export as a dict of plain numbers (what a checkpoint keeps).  Synchronises."""
        eng, st = self._engine, _lib.StepGuardState()
        _lib.check(eng.lib.fv_step_guard_export(eng.h, self.handle(), C.byref(st)), "fv_step_guard_export", eng.h)
        return {k: (float(getattr(st, k)) if k in ("last_inv_delta", "flag") else int(getattr(st, k))) for k in STATE_KEYS}

    def load_state(self, state: Dict) -> None:
        """fv_step_guard_import.  Synchronises."""
        eng = self._engine
        st = _lib.StepGuardState(*[(float(state[k]) if k in ("last_inv_delta", "flag") else int(state[k])) for k in STATE_KEYS])
        _lib.check(eng.lib.fv_step_guard_import(eng.h, self.handle(), C.byref(st)), "fv_step_guard_import", eng.h)

    def close(self) -> None:
        h, self._h, self._flag = getattr(self, "_h", None), None, None
        if h and getattr(self._engine, "h", None):      # (after the engine's fv_destroy only the host record is left: dropped with this object)
            _lib.check(self._engine.lib.fv_step_guard_destroy(self._engine.h, h), "fv_step_guard_destroy", self._engine.h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
