"""Exponential moving average (EMA) of the trainable weights, the parts that need no device: the options, their environment twins and the schedule of the
weight the fused step receives (include/fastvla_hip.h fv_adamw_clip_step_ema: ema <- ema + w (p_new - ema), w = 1 - decay).

Options (what a checkpoint records and a resume compares):
  decay         the average's decay d in [0, 1)                                                   FASTVLA_EMA_DECAY="0.999"   (alone it switches EMA on)
  warmup        ramp the decay up from the first update, d_t = min(d, (1 + tau) / (10 + tau))      FASTVLA_EMA_WARMUP="1"
  update_after  optimiser updates during which the average just follows the live weights (w = 1)   FASTVLA_EMA_UPDATE_AFTER="0"
with tau = t - update_after and t AdamW's own 1-based step.  The warm-up is the one of Diffusion Policy / LeRobot's EMAModel with inv_gamma 1, power 1
restated on the update count: without it the average would remember the initial weights for ~1 / (1 - d) updates, longer than many fine-tunes run."""
from __future__ import annotations

import math
import os
import struct
from typing import Dict, Optional

OPTION_KEYS = ("decay", "warmup", "update_after")
DEFAULTS = {"decay": 0.999, "warmup": True, "update_after": 0}
_TRUE, _FALSE = ("1", "true", "yes", "on"), ("0", "false", "no", "off")


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def normalize_options(decay=0.999, warmup=True, update_after=0) -> Dict:
    """-> {"decay": float, "warmup": bool, "update_after": int}.  ValueError: a decay outside [0, 1) or not a number, a warmup that is no boolean, a negative
    or fractional update_after."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"ema decay must be a number in [0, 1), got {decay!r}") from None
    if not (math.isfinite(d) and 0.0 <= d < 1.0):
        raise ValueError(f"ema decay must be in [0, 1), got {decay!r}")
    if not isinstance(warmup, (bool, int)) or warmup not in (0, 1):
        raise ValueError(f"ema warmup must be a boolean, got {warmup!r}")
    try:
        ua = int(update_after)
        if isinstance(update_after, bool) or ua != float(update_after) or ua < 0:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"ema update_after must be an integer >= 0, got {update_after!r}") from None
    return {"decay": d, "warmup": bool(warmup), "update_after": ua}


def _env_values(environ=None) -> Dict:
    """the twins that are set, parsed (unset and empty are the same)"""
    env = os.environ if environ is None else environ
    get = lambda k: (env.get(k) or "").strip()   # noqa: E731
    kw: Dict = {}
    if get("FASTVLA_EMA_DECAY"):
        kw["decay"] = get("FASTVLA_EMA_DECAY")
    raw = get("FASTVLA_EMA_WARMUP").lower()
    if raw:
        if raw not in _TRUE + _FALSE:
            raise ValueError(f"FASTVLA_EMA_WARMUP must be one of {', '.join(_TRUE + _FALSE)}, got '{raw}'")
        kw["warmup"] = raw in _TRUE
    raw = get("FASTVLA_EMA_UPDATE_AFTER")
    if raw:
        try:
            kw["update_after"] = int(raw)
        except ValueError:
            raise ValueError(f"FASTVLA_EMA_UPDATE_AFTER must be an integer >= 0, got '{raw}'") from None
    return kw


def options_from_env(environ=None) -> Optional[Dict]:
    """FASTVLA_EMA_DECAY, FASTVLA_EMA_WARMUP, FASTVLA_EMA_UPDATE_AFTER -> normalize_options' dict, or None when FASTVLA_EMA_DECAY is not set: the decay alone
    switches EMA on, the other two only shape it.  Malformed values raise ValueError."""
    kw = _env_values(environ)
    return normalize_options(**kw) if "decay" in kw else None


def resolve_options(decay=None, warmup=None, update_after=None, environ=None) -> Dict:
    """what enable_ema(...) runs with: per option the explicit argument, else its environment twin, else the default"""
    kw = _env_values(environ)
    for k, v in (("decay", decay), ("warmup", warmup), ("update_after", update_after)):
        if v is not None:
            kw[k] = v
    return normalize_options(**kw)


def ema_decay(options: Dict, t: int) -> float:
    """d_t of optimiser update t (1-based); only defined past update_after"""
    tau = int(t) - int(options["update_after"])
    if tau < 1:
        raise ValueError(f"update {t} is not past update_after = {options['update_after']}")
    d = float(options["decay"])
    return min(d, (1.0 + tau) / (10.0 + tau)) if options["warmup"] else d


def ema_weight(options: Dict, t: int) -> float:
    """the float32 weight w = 1 - d_t the kernel receives at optimiser update t (1-based, AdamW's own step): 1 up to update_after (the average IS the live
    weights), then float32(1 - d_t) with the subtraction in double"""
    if int(t) < 1:
        raise ValueError(f"optimiser updates count from 1, got {t}")
    if int(t) <= int(options["update_after"]):
        return 1.0
    return _f32(1.0 - ema_decay(options, t))
