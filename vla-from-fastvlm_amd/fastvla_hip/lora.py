"""LoRA mode of backbone training, the parts that need no device: target names and their bit mask (include/fastvla_hip.h fv_lora_target), argument checks,
the environment twins, a host-side mirror of fv_train_lora_layout (so a layout can be inspected, and the C side checked, without a handle) and PEFT's
initialisation of the adapters.

Two variants (fv_train_lora_begin_ex's flags): `rslora` -- rank-stabilised scaling, s = alpha / sqrt(rank) -- and `dora` -- weight-decomposed LoRA, PEFT's
use_dora: W' = diag(m / ||V||_row) V over V = W0 + s B A with a trained magnitude m per output row ("...lora_magnitude_vector.weight", 1 x out, behind each
target's lora_B).  Both keys appear in a configuration ONLY when true, so a plain run's configuration, adapter file and hip_extras.json are what they were."""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from .arch import ModelConfig

TARGETS: Tuple[str, ...] = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")   # bit i of the mask = TARGETS[i]
_MODULE = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
MAX_RANK = 64
HEAD_KEYS = ("state_projection.0.weight", "state_projection.0.bias", "state_projection.1.weight", "state_projection.1.bias", "fusion.0.weight", "fusion.0.bias",
             "fusion.1.weight", "fusion.1.bias", "fusion.4.weight", "fusion.4.bias", "action_head.weight", "action_head.bias")


def parse_targets(targets: Union[None, str, Iterable[str]]) -> Tuple[str, ...]:
    """None / "all" -> all seven; a comma-separated string or an iterable of names ("q_proj" or the short "q") -> the names in canonical order."""
    if targets is None:
        return TARGETS
    if isinstance(targets, str):
        if targets.strip().lower() in ("", "all"):
            return TARGETS
        targets = [t for t in targets.replace(" ", "").split(",") if t]
    got = set()
    for t in targets:
        name = t if t.endswith("_proj") else t + "_proj"
        if name not in TARGETS:
            raise ValueError(f"unknown LoRA target '{t}' (have {', '.join(TARGETS)})")
        got.add(name)
    if not got:
        raise ValueError("LoRA needs at least one target matrix")
    return tuple(t for t in TARGETS if t in got)


def target_mask(targets: Union[None, str, Iterable[str]]) -> int:
    return sum(1 << TARGETS.index(t) for t in parse_targets(targets))


def targets_of_mask(mask: int) -> Tuple[str, ...]:
    return tuple(t for i, t in enumerate(TARGETS) if mask >> i & 1)


FLAG_DORA, FLAG_RSLORA = 1, 2      # include/fastvla_hip.h fv_lora_flags
VARIANT_KEYS = ("dora", "rslora")


def _flag(name: str, v) -> bool:
    if isinstance(v, bool) or v is None:
        return bool(v)
    if isinstance(v, int) and v in (0, 1):
        return bool(v)
    raise ValueError(f"{name} must be a bool, got {v!r}")


def check_config(rank, alpha=None, targets=None, tower: bool = False, dora=False, rslora=False) -> Dict:
    """-> {"rank", "alpha", "targets"} with the defaults filled in (alpha = rank, all seven targets), plus "dora": True / "rslora": True ONLY when asked for
    (a plain configuration keeps exactly its three keys); raises ValueError on anything the library would refuse."""
    if isinstance(rank, bool) or int(rank) != rank:
        raise ValueError(f"lora_rank must be an integer, got {rank!r}")
    rank = int(rank)
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"lora_rank must be in 1 .. {MAX_RANK}, got {rank}")
    alpha = float(rank if alpha is None else alpha)
    if not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError(f"lora_alpha must be positive and finite, got {alpha}")
    if tower:
        raise ValueError("LoRA adapters go with a frozen vision tower: lora_rank and tower=True cannot be combined")
    cfg = {"rank": rank, "alpha": alpha, "targets": list(parse_targets(targets))}
    if _flag("lora_dora", dora):
        cfg["dora"] = True
    if _flag("lora_rslora", rslora):
        cfg["rslora"] = True
    return cfg


def variants_of(cfg: Optional[Dict]) -> Dict:
    """the variant keys of a configuration (or of a record that may predate them) as keyword arguments: {} for plain LoRA"""
    return {k: True for k in VARIANT_KEYS if cfg and cfg.get(k)}


def flags_of(cfg: Dict) -> int:
    return (FLAG_DORA if cfg.get("dora") else 0) | (FLAG_RSLORA if cfg.get("rslora") else 0)


def scale_of(cfg: Dict) -> float:
    """s of W0 + s B A: alpha / rank, or alpha / sqrt(rank) under rsLoRA"""
    return cfg["alpha"] / math.sqrt(cfg["rank"]) if cfg.get("rslora") else cfg["alpha"] / cfg["rank"]


def _env_flag(env, name: str) -> bool:
    raw = (env.get(name) or "").strip()
    if raw in ("", "0"):
        return False
    if raw == "1":
        return True
    raise ValueError(f"{name} must be 0 or 1, got '{raw}'")


def variants_from_env(environ=None) -> Dict:
    """FASTVLA_LORA_DORA / FASTVLA_LORA_RSLORA ("1" on; unset / empty / "0" off; anything else raises) -> {"dora": True} / {"rslora": True} / both / {}"""
    env = os.environ if environ is None else environ
    out = {}
    if _env_flag(env, "FASTVLA_LORA_DORA"):
        out["dora"] = True
    if _env_flag(env, "FASTVLA_LORA_RSLORA"):
        out["rslora"] = True
    return out


def config_from_env(environ=None) -> Optional[Dict]:
    """FASTVLA_LORA_RANK (unset / empty / 0: no LoRA), FASTVLA_LORA_ALPHA, FASTVLA_LORA_TARGETS (comma-separated), FASTVLA_LORA_DORA / FASTVLA_LORA_RSLORA
    (0 / 1) -> check_config's dict or None.  A variant without a rank raises."""
    env = os.environ if environ is None else environ
    raw = (env.get("FASTVLA_LORA_RANK") or "").strip()
    var = variants_from_env(env)
    if raw in ("", "0"):
        if var:
            raise ValueError("FASTVLA_LORA_DORA / FASTVLA_LORA_RSLORA need a rank (FASTVLA_LORA_RANK)")
        return None
    try:
        rank = int(raw)
    except ValueError:
        raise ValueError(f"FASTVLA_LORA_RANK must be an integer, got '{raw}'") from None
    alpha = (env.get("FASTVLA_LORA_ALPHA") or "").strip()
    return check_config(rank, float(alpha) if alpha else None, env.get("FASTVLA_LORA_TARGETS") or None, **var)


def direct_from_env(environ=None) -> bool:
    """FASTVLA_LORA_DIRECT: "1" -> the direct LoRA backward (fv_train_lora_forward_backward); unset / empty / "0" -> the projected one; anything else raises.
    A property of the run, not of the adapters: it is no part of config_from_env's dict."""
    env = os.environ if environ is None else environ
    raw = (env.get("FASTVLA_LORA_DIRECT") or "").strip()
    if raw in ("", "0"):
        return False
    if raw == "1":
        return True
    raise ValueError(f"FASTVLA_LORA_DIRECT must be 0 or 1, got '{raw}'")


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def logical_shapes(model: ModelConfig) -> Dict[str, Tuple[int, int]]:
    """target -> (out, in) of the logical matrix"""
    l = model.llm
    qd, kd = l.heads * l.head_dim, l.kv_heads * l.head_dim
    return {"q_proj": (qd, l.hidden), "k_proj": (kd, l.hidden), "v_proj": (kd, l.hidden), "o_proj": (l.hidden, qd),
            "gate_proj": (l.inter, l.hidden), "up_proj": (l.inter, l.hidden), "down_proj": (l.hidden, l.inter)}


def lora_layout(model: ModelConfig, rank: int, targets=None, *, state_dim: int = 14, action_dim: int = 14, hidden_dim: int = 1024, fusion_dim: int = 1024,
                dora: bool = False, flow_time_dim: int = 0):
    """The trainable flat buffer of LoRA mode, as fv_train_lora_layout reports it: -> (tensors, total_numel), tensors = dicts with name, offset, numel, rows,
    cols, bucket, packing (always 0).  [ head | projector | layer 0 adapters .. ]: every tensor starts on a multiple of 4 floats.  dora: each target's
    lora_magnitude_vector (1 x out) behind its lora_B.  flow_time_dim = E > 0: the flow head, whose fusion.0 reads action_dim + E more columns."""
    names = parse_targets(targets)
    H, CO = model.llm.hidden, model.tower.out_dim
    ds, da, hid, fus = state_dim, action_dim, hidden_dim, fusion_dim
    shapes = [(1, ds), (1, ds), (hid, ds), (1, hid), (fus, H + hid + (da + flow_time_dim if flow_time_dim else 0)), (1, fus), (1, fus), (1, fus), (fus, fus), (1, fus), (da, fus), (1, da)]
    out: List[Dict] = []
    off = 0

    def add(name, rows, cols, bucket):
        nonlocal off
        out.append(dict(name=name, offset=off, numel=rows * cols, rows=rows, cols=cols, bucket=bucket, packing=0))
        off += _pad4(rows * cols)

    for k, (r, c) in zip(HEAD_KEYS, shapes):
        add(k, r, c, 0)
    add("model.mm_projector.0.weight", H, CO, 1)
    add("model.mm_projector.0.bias", 1, H, 1)
    add("model.mm_projector.2.weight", H, H, 1)
    add("model.mm_projector.2.bias", 1, H, 1)
    shp = logical_shapes(model)
    for l in range(model.llm.layers):
        for t in names:
            o, i = shp[t]
            pre = f"model.layers.{l}.{_MODULE[t]}.{t}"
            add(pre + ".lora_A.weight", rank, i, 3 + l)
            add(pre + ".lora_B.weight", o, rank, 3 + l)
            if dora:
                add(pre + ".lora_magnitude_vector.weight", 1, o, 3 + l)
    return out, off


def init_adapters(flat: torch.Tensor, tensors: Sequence[Dict], seed: int = 0) -> None:
    """PEFT's initialisation into the trainable buffer: lora_A Kaiming-uniform with a = sqrt(5) (U(-1/sqrt(in), 1/sqrt(in))) from a seeded CPU generator, in
    layout order, lora_B = 0 -- so the adapted model starts as the base model.  (DoRA's magnitudes are not touched: FastVLAEngine.train_lora_init_magnitude
    computes them on the device from the master.)"""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    for t in tensors:
        v = flat[t["offset"]: t["offset"] + t["numel"]]
        if t["name"].endswith(".lora_A.weight"):
            bound = 1.0 / math.sqrt(t["cols"])
            v.copy_(((torch.rand(t["numel"], generator=g) * 2 - 1) * bound).to(flat.device))
        elif t["name"].endswith(".lora_B.weight"):
            v.zero_()


def adapter_views(flat: torch.Tensor, tensors: Sequence[Dict]) -> Dict[str, torch.Tensor]:
    """name -> (rows, cols) view into the trainable buffer, adapters only"""
    return {t["name"]: flat[t["offset"]: t["offset"] + t["numel"]].view(t["rows"], t["cols"]) for t in tensors if ".lora_" in t["name"]}
