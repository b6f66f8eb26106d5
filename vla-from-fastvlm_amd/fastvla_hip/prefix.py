"""Host side of the flow head's action-prefix conditioning (FastVLAEngine.set_head_flow_prefix; fv_head_set_flow_prefix): the delay table, the argument
checks that run before any engine exists, and the widening of a plain flow head's fusion.0.weight.  No GPU, no library call.

A delay d in 0 .. D is drawn per head row during training: the first d steps of the chunk reach the network clean and stay out of the loss.  The library
draws it with an integer compare, d = the smallest j with (z >> 8) < thresholds[j], z a 32-bit Philox word; thresholds are the cumulative distribution in
units of 2^-24."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

DELAY_DISTS = ("uniform", "exp")
UNIT = 1 << 24
FUSION0 = "fusion.0.weight"


def delay_probabilities(max_delay: int, dist: str = "uniform", rate: float = 0.0) -> List[float]:
    """p_0 .. p_D in double: "uniform" p_d = 1 / (D + 1); "exp" p_d proportional to exp(-rate d)"""
    D = check_max_delay_value(max_delay)
    if dist not in DELAY_DISTS:
        raise ValueError(f"flow_prefix_delay_dist must be one of {list(DELAY_DISTS)}, got {dist!r}")
    if dist == "uniform":
        return [1.0 / (D + 1)] * (D + 1)
    rate = float(rate)
    if not math.isfinite(rate) or rate < 0.0:
        raise ValueError(f"flow_prefix_delay_rate must be finite and >= 0, got {rate!r}")
    w = [math.exp(-rate * d) for d in range(D + 1)]
    tot = math.fsum(w)
    return [x / tot for x in w]


def delay_thresholds(max_delay: int, dist: str = "uniform", rate: float = 0.0) -> List[int]:
    """D + 1 non-decreasing integers, thresholds[j] = round(2^24 (p_0 + .. + p_j)), the last one exactly 2^24"""
    p = delay_probabilities(max_delay, dist, rate)
    thr, run = [], 0.0
    for x in p:
        run += x
        thr.append(min(UNIT, int(round(run * UNIT))))
    thr[-1] = UNIT
    for j in range(1, len(thr)):
        thr[j] = max(thr[j], thr[j - 1])
    return thr


def table_probabilities(thresholds) -> List[float]:
    """the probabilities the integer table realises exactly: (thresholds[j] - thresholds[j - 1]) / 2^24"""
    thr = [int(x) for x in thresholds]
    return [(b - a) / UNIT for a, b in zip([0] + thr[:-1], thr)]


def check_max_delay_value(max_delay) -> int:
    if isinstance(max_delay, bool) or not isinstance(max_delay, int) and not (isinstance(max_delay, float) and max_delay == int(max_delay)):
        raise ValueError(f"flow_prefix_max_delay must be an integer >= 1, got {max_delay!r}")
    if int(max_delay) < 1:
        raise ValueError(f"flow_prefix_max_delay must be an integer >= 1, got {max_delay!r}")
    return int(max_delay)


def check_prefix_config(max_delay, *, action_head: str, chunk_size: int, temporal_ensemble_coeff=None, dist: str = "uniform", rate: float = 0.0) -> Optional[dict]:
    """-> None when max_delay is None (the mode is off), else {"chunk", "max_delay", "dist", "rate", "thresholds"}.  Every refusal is a ValueError that names
    both settings, raised from plain values: no engine is needed to call it."""
    if max_delay is None:
        return None
    D = check_max_delay_value(max_delay)
    if action_head != "flow":
        raise ValueError(f"flow_prefix_max_delay={D} needs action_head='flow', got action_head={action_head!r}")
    if int(chunk_size) == 1:
        raise ValueError(f"flow_prefix_max_delay={D} needs an action chunk, got chunk_size=1")
    if D >= int(chunk_size):
        raise ValueError(f"flow_prefix_max_delay={D} must be below chunk_size={int(chunk_size)}")
    if temporal_ensemble_coeff is not None:
        raise ValueError(f"flow_prefix_max_delay={D} cannot be combined with temporal_ensemble_coeff={temporal_ensemble_coeff!r}: "
                         "a pinned prefix and an ensembled action are two answers to the same chunk overlap")
    return dict(chunk=int(chunk_size), max_delay=D, dist=dist, rate=float(rate), thresholds=delay_thresholds(D, dist, rate))


def check_inference_delay(inference_delay, max_delay: int) -> int:
    d = int(inference_delay)
    if d < 0 or d > int(max_delay):
        raise ValueError(f"inference_delay={d} outside 0 .. flow_prefix_max_delay={int(max_delay)}")
    return d


def extras_record(cfg: Optional[dict]) -> Dict[str, object]:
    """the fields the prefix mode adds to the `action_head` record of hip_extras.json (nothing when the mode is off)"""
    if not cfg:
        return {}
    return {"prefix_max_delay": int(cfg["max_delay"]), "prefix_delay_dist": str(cfg["dist"]), "prefix_delay_rate": float(cfg["rate"])}


def widen_flow_state_dict(state_dict: dict, chunk: int, key: str = FUSION0) -> dict:
    """a copy of a plain flow head's state dict whose fusion.0.weight has `chunk` zero columns appended: the prefix-width head that computes the plain head's
    velocity for m = 0, so an existing flow checkpoint can be fine-tuned into a prefix head.  `key`: the entry to widen (a suffix match finds prefixed names)"""
    import torch

    names = [k for k in state_dict if k == key or k.endswith("." + key)]
    if len(names) != 1:
        raise ValueError(f"expected exactly one {key!r} in the state dict, found {names}")
    if int(chunk) < 2:
        raise ValueError(f"chunk must be >= 2, got {chunk!r}")
    out = dict(state_dict)
    w = state_dict[names[0]]
    out[names[0]] = torch.cat([w, torch.zeros(w.shape[0], int(chunk), dtype=w.dtype, device=w.device)], dim=1)
    return out
