"""On-device image augmentation of the training input pipeline (include/fastvla_hip.h fv_augment_draw / fv_preprocess_augmented), the parts that need no
device: the options, their environment twins, the preset and the ctypes mirrors of the two structs.

Options: five ranges (lo, hi), a single number meaning (v, v):
  crop_area    fraction of the image's area the crop window covers            default (1, 1)
  crop_ratio   the window's aspect relative to the image's own, log-uniform   default (1, 1)
  brightness   factor b                                                       default (1, 1)
  contrast     factor c, about the gray mean of the whole source image        default (1, 1)
  saturation   factor s                                                       default (1, 1)
Colour is brightness -> contrast -> saturation in this fixed order with ONE clamp at the end: v' = clamp(b c (s v + (1 - s) gray(v)) + (1 - c) b mu, 0,
value_max).  torchvision's ColorJitter applies its factors in a random order and clamps after each; this does neither.

Environment twins (an explicit argument beats its twin):
  FASTVLA_IMAGE_AUG        "1" = the preset `default`, "0" / unset = off, or "crop_area=0.9:0.9,brightness=0.8:1.2,..." (unnamed ranges stay (1, 1))
  FASTVLA_IMAGE_AUG_SEED   the seed (default 0)"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional, Tuple

OPTION_KEYS: Tuple[str, ...] = ("crop_area", "crop_ratio", "brightness", "contrast", "saturation")
IDENTITY: Dict[str, Tuple[float, float]] = {k: (1.0, 1.0) for k in OPTION_KEYS}
# OpenVLA's fine-tuning recipe without hue: a 90 %-area crop at the image's own aspect, brightness / contrast / saturation in 0.8 .. 1.2
PRESETS: Dict[str, Dict[str, Tuple[float, float]]] = {
    "default": {"crop_area": (0.9, 0.9), "crop_ratio": (1.0, 1.0), "brightness": (0.8, 1.2), "contrast": (0.8, 1.2), "saturation": (0.8, 1.2)},
}


class AugmentSample(C.Structure):      # fv_augment_sample: 80 bytes
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("cw", C.c_float), ("ch", C.c_float), ("m", C.c_float * 9), ("o", C.c_float * 3),
                ("colour", C.c_int32), ("pad", C.c_int32 * 3)]


class AugmentConfig(C.Structure):      # fv_augment_config: 40 bytes
    _fields_ = [(k, C.c_float * 2) for k in OPTION_KEYS]


SAMPLE_FLOATS = C.sizeof(AugmentSample) // 4      # a table is a (B, 20) fp32 tensor; column 16 holds the int32 `colour`


def _range(name: str, v) -> Tuple[float, float]:
    try:
        if isinstance(v, (int, float)):
            lo = hi = float(v)
        else:
            seq = tuple(v)
            if len(seq) != 2:
                raise TypeError
            lo, hi = float(seq[0]), float(seq[1])
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or a pair (lo, hi), got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{name} must be finite, got {v!r}")
    if lo > hi:
        raise ValueError(f"{name}: lo > hi ({lo} > {hi})")
    if name in ("crop_area", "crop_ratio"):
        if lo <= 0.0:
            raise ValueError(f"{name} must be positive, got {v!r}")
        if name == "crop_area" and hi > 1.0:
            raise ValueError(f"crop_area is a fraction of the image's area: hi must be <= 1, got {v!r}")
    elif lo < 0.0:
        raise ValueError(f"{name} must be >= 0, got {v!r}")
    return (lo, hi)


def normalize_options(crop_area=None, crop_ratio=None, brightness=None, contrast=None, saturation=None) -> Dict[str, Tuple[float, float]]:
    """-> all five ranges in canonical form ((lo, hi) floats; an option left None is (1, 1)): what a checkpoint records and a resume compares.
    Raises ValueError: lo > hi, a non-positive area or ratio, an area above 1, a negative or non-finite factor."""
    given = dict(crop_area=crop_area, crop_ratio=crop_ratio, brightness=brightness, contrast=contrast, saturation=saturation)
    return {k: IDENTITY[k] if given[k] is None else _range(k, given[k]) for k in OPTION_KEYS}


def preset(name: str = "default") -> Dict[str, Tuple[float, float]]:
    if name not in PRESETS:
        raise ValueError(f"unknown augmentation preset '{name}' (have {', '.join(PRESETS)})")
    return normalize_options(**PRESETS[name])


def is_identity(options: Optional[Dict]) -> bool:
    """True when every range is (1, 1): such a configuration draws identity rows, and the augmented call gives fv_preprocess's bits"""
    return not options or all(tuple(options.get(k, (1.0, 1.0))) == (1.0, 1.0) for k in OPTION_KEYS)


def options_from_env(environ=None) -> Optional[Dict[str, Tuple[float, float]]]:
    """FASTVLA_IMAGE_AUG -> normalize_options' dict, or None when unset / empty / "0".  Malformed values raise ValueError."""
    env = os.environ if environ is None else environ
    raw = (env.get("FASTVLA_IMAGE_AUG") or "").strip()
    if raw in ("", "0"):
        return None
    if raw == "1":
        return preset("default")
    kw: Dict = {}
    for item in [s for s in raw.replace(" ", "").split(",") if s]:
        k, eq, v = item.partition("=")
        if not eq or not k or not v:
            raise ValueError(f"FASTVLA_IMAGE_AUG: '{item}' is not name=lo:hi")
        if k not in OPTION_KEYS:
            raise ValueError(f"FASTVLA_IMAGE_AUG: unknown option '{k}' (have {', '.join(OPTION_KEYS)})")
        if k in kw:
            raise ValueError(f"FASTVLA_IMAGE_AUG names '{k}' twice")
        lo, colon, hi = v.partition(":")
        try:
            kw[k] = (float(lo), float(hi)) if colon else float(lo)
        except ValueError:
            raise ValueError(f"FASTVLA_IMAGE_AUG: '{item}' is not name=lo:hi") from None
    return normalize_options(**kw)


def seed_from_env(environ=None) -> int:
    env = os.environ if environ is None else environ
    raw = (env.get("FASTVLA_IMAGE_AUG_SEED") or "").strip()
    if not raw:
        return 0
    try:
        seed = int(raw)
    except ValueError:
        raise ValueError(f"FASTVLA_IMAGE_AUG_SEED must be an integer, got {raw!r}") from None
    if seed < 0:
        raise ValueError(f"FASTVLA_IMAGE_AUG_SEED must be >= 0, got {raw!r}")
    return seed


def resolve(crop_area=None, crop_ratio=None, brightness=None, contrast=None, saturation=None, seed=None, environ=None):
    """What enable_image_augmentation() runs with -> (options, seed).  With no explicit range at all the environment twin decides (absent: the preset
    `default`); an explicit range beats the twin's value for that option, the twin fills the others."""
    given = {k: v for k, v in dict(crop_area=crop_area, crop_ratio=crop_ratio, brightness=brightness, contrast=contrast, saturation=saturation).items()
             if v is not None}
    base = options_from_env(environ)
    if base is None:
        base = preset("default") if not given else dict(IDENTITY)
    opts = {**base, **{k: v for k, v in normalize_options(**given).items() if k in given}}
    return opts, (seed_from_env(environ) if seed is None else int(seed))


def record(options: Dict) -> Dict:
    """the JSON-friendly form (lists) of normalize_options' dict"""
    return {k: [float(options[k][0]), float(options[k][1])] for k in OPTION_KEYS}


def from_record(rec: Dict) -> Dict[str, Tuple[float, float]]:
    return normalize_options(**{k: tuple(rec[k]) for k in OPTION_KEYS if k in rec})


def config_struct(options: Dict) -> AugmentConfig:
    cfg = AugmentConfig()
    for k in OPTION_KEYS:
        lo, hi = options.get(k, (1.0, 1.0))
        getattr(cfg, k)[0], getattr(cfg, k)[1] = float(lo), float(hi)
    return cfg
