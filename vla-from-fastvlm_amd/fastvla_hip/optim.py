"""Parameter groups for the fused clip + AdamW step (include/fastvla_hip.h fv_adamw_group / fv_adamw_clip_step_groups), the parts that need no device:
the options, their environment twins and the group table of a layout.

A layout is what fv_train_layout / fv_train_lora_layout report (FastVLAEngine.train_layout() / train_lora_layout(), or lora.lora_layout() without a handle):
dicts with name, offset, numel, rows, cols, bucket.  Its tensors fall into SECTIONS by bucket -- "head" (bucket 0), "projector" (1), "embedding" (2),
"decoder" (3 .. 3 + L: the L layers and the final norm), "tower" (the buckets above) -- except the adapters ("...lora_A / lora_B / lora_magnitude_vector"),
which form the section "adapters" whatever layer they sit in.  One CLASS cuts across the sections: "vectors", every tensor with rows == 1 (norm weights,
biases, layer scales, DoRA magnitudes).

Options (all optional; none set = the single-group step fv_adamw_clip_step, bit for bit):
  lr_scales        {section: factor} on the learning rate                                   FASTVLA_LR_SCALES="decoder=0.1,tower=0.1"
  no_decay         sections and / or "vectors" whose weight decay is 0                      FASTVLA_NO_DECAY="vectors"
  layer_decay      d: decoder layer l of L (and its adapters) x d^(L-1-l), embedding x d^L  FASTVLA_LAYER_DECAY="0.9"
  lora_plus_ratio  lora_B's learning rate over lora_A's (LoRA+)                             FASTVLA_LORA_PLUS_RATIO="16"
  freeze           sections and / or "vectors" left untouched (no update, not in the norm)  FASTVLA_FREEZE="embedding"
Factors multiply."""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

SECTIONS: Tuple[str, ...] = ("head", "projector", "embedding", "decoder", "tower", "adapters")
VECTORS = "vectors"
OPTION_KEYS: Tuple[str, ...] = ("lr_scales", "no_decay", "layer_decay", "lora_plus_ratio", "freeze")
_ADAPTER_MARKS = (".lora_A.", ".lora_B.", ".lora_magnitude_vector.")


def _is_adapter(name: str) -> bool:
    return any(m in name for m in _ADAPTER_MARKS)


def _names(what: str, v: Union[None, str, Iterable[str]]) -> Tuple[str, ...]:
    if v is None:
        return ()
    if isinstance(v, str):
        v = [s for s in v.replace(" ", "").split(",") if s]
    out = []
    for s in v:
        if s not in SECTIONS and s != VECTORS:
            raise ValueError(f"{what}: unknown section '{s}' (have {', '.join(SECTIONS)} and the class '{VECTORS}')")
        if s not in out:
            out.append(s)
    return tuple(sorted(out))


def _factor(what: str, v) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, got {v!r}") from None
    if not (math.isfinite(f) and f >= 0.0):
        raise ValueError(f"{what} must be finite and >= 0, got {v!r}")
    return f


def normalize_options(lr_scales=None, no_decay=(), layer_decay=None, lora_plus_ratio=None, freeze=()) -> Dict:
    """-> the options in canonical form, ONLY the ones that are set ({} = the single-group step): what a checkpoint records and a resume compares.
    Raises ValueError on an unknown section or a factor that is negative or not finite."""
    out: Dict = {}
    if lr_scales:
        sc = {}
        for k, v in dict(lr_scales).items():
            if k not in SECTIONS:
                raise ValueError(f"lr_scales: unknown section '{k}' (have {', '.join(SECTIONS)})")
            sc[k] = _factor(f"lr_scales['{k}']", v)
        out["lr_scales"] = {k: sc[k] for k in sorted(sc)}
    nd = _names("no_decay", no_decay)
    if nd:
        out["no_decay"] = list(nd)
    if layer_decay is not None:
        d = _factor("layer_decay", layer_decay)
        if d <= 0.0:
            raise ValueError(f"layer_decay must be positive, got {layer_decay!r}")
        out["layer_decay"] = d
    if lora_plus_ratio is not None:
        out["lora_plus_ratio"] = _factor("lora_plus_ratio", lora_plus_ratio)
    fr = _names("freeze", freeze)
    if fr:
        out["freeze"] = list(fr)
    return out


def explicit_kwargs(opts: Optional[Dict]) -> Dict:
    """normalize_options' dict as enable_backbone_training's keywords with every list / dict option explicit (an unset one as its empty value), so that no
    environment twin fills one in: what a resume passes to bring a checkpointed run's options back"""
    o = dict(opts or {})
    return {"lr_scales": dict(o.get("lr_scales", {})), "no_decay": tuple(o.get("no_decay", ())), "freeze": tuple(o.get("freeze", ())),
            **({"layer_decay": o["layer_decay"]} if "layer_decay" in o else {}), **({"lora_plus_ratio": o["lora_plus_ratio"]} if "lora_plus_ratio" in o else {})}


def options_from_env(environ=None) -> Dict:
    """FASTVLA_LR_SCALES ("section=factor,..."), FASTVLA_NO_DECAY / FASTVLA_FREEZE (comma-separated sections or "vectors"), FASTVLA_LAYER_DECAY,
    FASTVLA_LORA_PLUS_RATIO -> normalize_options' dict ({} when none is set; unset and empty are the same).  Malformed values raise ValueError."""
    env = os.environ if environ is None else environ
    get = lambda k: (env.get(k) or "").strip()
    kw: Dict = {}
    raw = get("FASTVLA_LR_SCALES")
    if raw:
        sc = {}
        for item in [s for s in raw.replace(" ", "").split(",") if s]:
            k, eq, v = item.partition("=")
            if not eq or not k or not v:
                raise ValueError(f"FASTVLA_LR_SCALES: '{item}' is not section=factor")
            if k in sc:
                raise ValueError(f"FASTVLA_LR_SCALES names '{k}' twice")
            sc[k] = _factor(f"FASTVLA_LR_SCALES {k}", v)
        kw["lr_scales"] = sc
    if get("FASTVLA_NO_DECAY"):
        kw["no_decay"] = get("FASTVLA_NO_DECAY")
    if get("FASTVLA_FREEZE"):
        kw["freeze"] = get("FASTVLA_FREEZE")
    if get("FASTVLA_LAYER_DECAY"):
        kw["layer_decay"] = _factor("FASTVLA_LAYER_DECAY", get("FASTVLA_LAYER_DECAY"))
    if get("FASTVLA_LORA_PLUS_RATIO"):
        kw["lora_plus_ratio"] = _factor("FASTVLA_LORA_PLUS_RATIO", get("FASTVLA_LORA_PLUS_RATIO"))
    return normalize_options(**kw)


def decoder_layers(tensors: Sequence[Dict]) -> int:
    """L of a layout: the final norm sits in bucket 3 + L; a LoRA layout has no final norm, its last adapters sit in bucket 3 + L - 1"""
    for t in tensors:
        if t["name"] == "model.norm.weight":
            return int(t["bucket"]) - 3
    ad = [int(t["bucket"]) for t in tensors if _is_adapter(t["name"])]
    return max(ad) - 2 if ad else 0


def section_of(t: Dict, L: int) -> str:
    if _is_adapter(t["name"]):
        return "adapters"
    b = int(t["bucket"])
    return "head" if b == 0 else "projector" if b == 1 else "embedding" if b == 2 else "decoder" if b <= 3 + L else "tower"


def build_param_groups(tensors: Sequence[Dict], *, weight_decay: float, lr_scales=None, no_decay=(), layer_decay=None, lora_plus_ratio=None, freeze=(),
                       total: Optional[int] = None):
    """The group table of a layout -> (groups, names): groups = dicts of begin, end, lr_scale, weight_decay, frozen that tile [0, total) (total: the
    buffer's length; default the last tensor's end rounded up to 4), names = one label per group.  A tensor's group runs to the NEXT tensor's offset, so
    the padding behind it belongs to it; adjacent tensors with equal settings merge into one group.  Raises ValueError: unknown section, lora_plus_ratio
    over a layout without adapters, a tensor that does not start on a multiple of 4 floats, tensors out of order."""
    opt = normalize_options(lr_scales, no_decay, layer_decay, lora_plus_ratio, freeze)
    wd = _factor("weight_decay", weight_decay)
    if not tensors:
        raise ValueError("build_param_groups: empty layout")
    scales, nd, fr = opt.get("lr_scales", {}), set(opt.get("no_decay", ())), set(opt.get("freeze", ()))
    d, ratio = opt.get("layer_decay"), opt.get("lora_plus_ratio")
    if ratio is not None and not any(_is_adapter(t["name"]) for t in tensors):
        raise ValueError("lora_plus_ratio needs LoRA adapters: this layout has none")
    L = decoder_layers(tensors)
    end_all = (int(tensors[-1]["offset"]) + int(tensors[-1]["numel"]) + 3) // 4 * 4 if total is None else int(total)
    groups: List[Dict] = []
    spans: List[List[str]] = []
    if int(tensors[0]["offset"]) != 0:
        raise ValueError(f"the layout's first tensor starts at {tensors[0]['offset']}, not at 0")
    for i, t in enumerate(tensors):
        begin = int(t["offset"])
        end = int(tensors[i + 1]["offset"]) if i + 1 < len(tensors) else end_all
        if begin % 4 or end % 4:
            raise ValueError(f"{t['name']}: [{begin}, {end}) is not on multiples of 4 floats")
        if end < begin + int(t["numel"]):
            raise ValueError(f"{t['name']}: [{begin}, {begin + int(t['numel'])}) runs past the next tensor's offset {end}")
        sec = section_of(t, L)
        vec = int(t["rows"]) == 1
        f = scales.get(sec, 1.0)
        if d is not None:
            b = int(t["bucket"])
            if sec == "embedding":
                f *= d ** L
            elif sec in ("decoder", "adapters") and 3 <= b < 3 + L:
                f *= d ** (L - 1 - (b - 3))
        if ratio is not None and ".lora_B." in t["name"]:
            f *= ratio
        g = dict(begin=begin, end=end, lr_scale=float(f), weight_decay=0.0 if (sec in nd or (vec and VECTORS in nd)) else wd,
                 frozen=bool(sec in fr or (vec and VECTORS in fr)))
        last = groups[-1] if groups else None
        if last is not None and (last["lr_scale"], last["weight_decay"], last["frozen"]) == (g["lr_scale"], g["weight_decay"], g["frozen"]):
            last["end"] = end
            spans[-1].append(t["name"])
        else:
            groups.append(g)
            spans.append([t["name"]])
    names = [s[0] if len(s) == 1 else f"{s[0]} .. {s[-1]} ({len(s)} tensors)" for s in spans]
    return groups, names
