"""Load / write `policy_config.json` + `policy_state_dict.pt` (reference: src/vla_fastvlm/utils/checkpoint.py:14-47 reads them,
training/trainer.py:246-255 writes them).

Read side.  The 12 head tensors (`model.state_projection.*`, `model.fusion.*`, `model.action_head.*`) always come from the file.  A
checkpoint written by the REFERENCE also carries the whole VLM under `model.backbone.model.*` (the backbone is a submodule there, so
`state_dict()` includes it, and `load_state_dict` puts it back over whatever `from_pretrained` loaded): those tensors are handed to the
backbone (`FastVLMBackbone.load_backbone_state`: canonical keys = the reference's keys minus the prefix, training-form towers folded,
`lm_head.*` dropped) and packed into the engine instead of the ones `vlm_model_name` resolves to.  A checkpoint without them (what this
build writes by default: the frozen backbone is not duplicated next to every head) keeps the `vlm_model_name` weights.

Write side.  `save_policy_checkpoint(policy, dir, include_backbone=True)` writes the file the reference's own
`load_policy_from_checkpoint(strict=True)` accepts: head tensors + every VLM tensor under `model.backbone.model.*` (+ the tied
`lm_head.weight`)."""
from __future__ import annotations

import dataclasses
import json
from pathlib import Path

import torch

from ..fastvla import FastVLAConfig, FastVLAPolicy

BACKBONE_PREFIX = "model.backbone.model."
# run properties of THIS build that are not tensors of the reference's module tree: written beside the two reference files, never into them, so that the
# reference's strict `load_state_dict` / `FastVLAConfig(**payload)` accept a checkpoint of an unfrozen run as it is.  Keys: "splice_image_tokens"
# (the decoder was trained on [image tokens | text]: inference must run the same graph), "train_backbone", "train_tower", and -- only for a run with image
# augmentation on -- "augment" = {"options", "seed"} (what the training batches went through; inference never augments).
EXTRAS_FILE = "hip_extras.json"
# a LoRA run (enable_backbone_training(lora_rank=...)): the adapters, the mm_projector that trains beside them and {rank, alpha, targets} in a file of their
# own; EXTRAS_FILE names it under "lora" = {"rank", "alpha", "targets", "file", "direct"}, and a directory whose extras name adapters that are not there does not
# load.  "dora" / "rslora" (the adapters' variants) are there only when true: a plain run's record is what it always was, and a record without them is plain LoRA.
# "direct" records the run's backward mode (the direct LoRA backward; absent = projected): the default when loading has to switch LoRA mode on itself
# "action_chunk" = {"chunk_size", "n_action_steps", "loss", "beta"} -- only when something differs from (1, 1, "mse", 1.0): the head of a chunked policy is
# K * A wide, which the reference's config cannot say; a plain policy's extras file is byte for byte what it was
# (+ "temporal_ensemble_coeff", "dim_weights", "step_weights" -- each only when set: select_action's temporal ensembling and the weights of the chunk loss)
# "action_head" = {"type": "flow", "steps", "time_dim", "min_period", "max_period", "time_dist", "dist_a", "dist_b", "seed"} -- only for a flow-matching head
# ("time_dist" is the option's string: "uniform" | "logit_normal" | "beta:1.5,1.0"; + "time_range" = [lo, hi] and "time_stratify" = true -- each only when set)
# (FastVLAPolicy(action_head="flow")), whose fusion.0.weight is chunk_size * action_dim + time_dim columns wider than the regression head's
# (+ "prefix_max_delay", and "prefix_delay_dist" / "prefix_delay_rate" for information -- only for a head with action-prefix conditioning
# (flow_prefix_max_delay), whose fusion.0.weight has chunk_size more columns still)
# "action_head" = {"type": "bins", "bins", "range" (a list of [lo, hi] pairs: one, or one per action dimension), "sigma", "decode"} -- only for a binned head
# (FastVLAPolicy(action_head="bins")), whose action_head.weight has `bins` times the rows of the regression head's
LORA_FILE = "lora_adapters.pt"
SPLICE_KEY_MARK = ".splice_image_tokens"


def read_extras(checkpoint_dir) -> dict:
    f = Path(checkpoint_dir) / EXTRAS_FILE
    return json.loads(f.read_text()) if f.is_file() else {}
# state-dict keys of this build that exist only while their feature is on (so a default policy keeps exactly the reference's keys): folded
# dataset statistics (FastVLMBackbone._save_to_state_dict), and -- in files written by round 5 -- the spliced-sequence mode of an unfrozen run (now in EXTRAS_FILE)
EXTRA_STATE_MARKS = (".io_norm.", ".splice_image_tokens")


def optimizer_record(st: dict, un, global_step: int, update_step: int, augment: dict | None = None, ema: dict | None = None,
                     step_guard: dict | None = None) -> dict:
    """What Trainer writes to optimizer.pt: AdamW's moments and step, the loop's counters, and for an unfrozen run (`un`, training/unfrozen.py UnfrozenState) its
    trainable fp32 buffer and what it trains.  "optim" -- the parameter-group options of the run (fastvla_hip/optim.py) -- is there ONLY when one is set: a
    plain run's file is byte for byte what it was.  "augment" -- {options, seed, batches} of a run with image augmentation on
    (FastVLMBackbone.augmentation_record; batches = training batches STEPPED) -- likewise only when it is on.  "ema" -- {options, shadow, updates} of a run that
    keeps an EMA of its weights (policy.ema_record()) -- likewise.  "step_guard" -- {options, state} of a run with the step guard on
    (policy.step_guard_record()) -- likewise.  "flat" and the weight files beside this one are always the LIVE weights."""
    rec = {"m": st["m"].cpu(), "v": st["v"].cpu(), "step": st["step"], "global_step": global_step, "update_step": update_step}
    if augment is not None:
        rec["augment"] = dict(augment)
    if ema is not None:
        rec["ema"] = dict(ema)
    if step_guard is not None:
        rec["step_guard"] = dict(step_guard)
    if un is not None:
        # the fp32 MASTER of an unfrozen run: the VLM tensors of policy_state_dict.pt come back through the engine's bf16 operand copies, and a master
        # rebuilt from those has lost the low bits every later update (~1e-3 of a bf16 ulp) lives in
        rec["flat"] = un.trainable.cpu()     # (a LoRA run: head + projector + adapters; its frozen master is the base checkpoint)
        rec["train_backbone"], rec["train_tower"] = True, bool(un.train_tower)   # what the run trains comes back from the checkpoint, not from the environment
        if un.lora is not None:
            rec["lora"] = dict(un.lora)
        if getattr(un, "optim", None):
            rec["optim"] = dict(un.optim)
    return rec


def check_resume_optim(recorded, current) -> None:
    """A resumed run must step the way the checkpointed one did: other parameter-group options (a missing record = none) raise, naming both."""
    recorded, current = dict(recorded or {}), dict(current or {})
    if recorded != current:
        raise ValueError(f"optimizer.pt was written by a run with the optimiser options {recorded or 'none'}, this run uses {current or 'none'}: "
                         "resume with the checkpoint's options (lr_scales / no_decay / layer_decay / lora_plus_ratio / freeze or their FASTVLA_* twins)")


def check_resume_ema(recorded, current) -> None:
    """A resumed run must average the way the checkpointed one did: other EMA options raise ValueError, naming both (fastvla/ema_state.py)."""
    from ..fastvla.ema_state import check_resume_ema as _check
    _check(recorded, current)


# the weight files of a checkpoint directory: what `<suffix>-ema/` holds (written inside policy.ema_weights(): a plain deployable policy of the averaged weights)
EMA_SUFFIX = "-ema"


def check_head_width(state: dict, action_dim: int, chunk: dict, where="", head: dict | None = None) -> None:
    """the action head of the file against what policy_config.json and the extras records say: a wide head without a record does not load.  head: the file's
    "action_head" record (a binned head is `bins` times taller)"""
    w = state.get("model.action_head.weight")
    bins = int(head["bins"]) if head and head.get("type") == "bins" else 1
    want = int((chunk or {}).get("chunk_size", 1)) * int(action_dim) * bins
    if w is not None and w.shape[0] != want:
        raise ValueError(f"{where}: model.action_head.weight is {tuple(w.shape)}, but action_dim={action_dim} with "
                         f"{'chunk_size=' + str(chunk['chunk_size']) if chunk else 'no action_chunk record in ' + EXTRAS_FILE}"
                         f"{' and bins=' + str(bins) if bins > 1 else ''} asks for ({want}, {w.shape[1]})")


def check_action_head_shape(state: dict, policy, where="") -> None:
    """action_head.weight of the file against the policy's head: a binned checkpoint does not load into a regression or flow policy, nor the reverse"""
    w, own = state.get("model.action_head.weight"), policy.model.action_head.weight
    if w is not None and tuple(w.shape) != tuple(own.shape):
        raise ValueError(f"{where}: model.action_head.weight is {tuple(w.shape)} in the checkpoint and {tuple(own.shape)} in this policy, which was built with "
                         f"action_head='{getattr(policy, 'action_head', 'regression')}': a binned head's action_head has action_bins rows per action element -- "
                         f"build the policy with the action_head setting (action_bins, chunk_size) the checkpoint was trained with")


def check_fusion_width(state: dict, policy, where="") -> None:
    """fusion.0.weight of the file against the policy's head: a flow checkpoint does not load into a regression policy, nor the reverse"""
    w, own = state.get("model.fusion.0.weight"), policy.model.fusion[0].weight
    if w is not None and tuple(w.shape) != tuple(own.shape):
        raise ValueError(f"{where}: model.fusion.0.weight is {tuple(w.shape)} in the checkpoint and {tuple(own.shape)} in this policy, which was built with "
                         f"action_head='{getattr(policy, 'action_head', 'regression')}': a flow head's fusion.0 reads chunk_size * action_dim + flow_time_dim more "
                         f"columns than a regression head's, and a head with flow_prefix_max_delay chunk_size more than a plain flow head's (fastvla_hip.prefix."
                         f"widen_flow_state_dict widens a plain flow checkpoint) -- build the policy with the action_head setting (flow_time_dim, flow_prefix_max_delay) "
                         f"the checkpoint was trained with")


def load_policy_from_checkpoint(checkpoint_dir: str, device: torch.device | None = None) -> FastVLAPolicy:
    root = Path(checkpoint_dir)
    cfg_path, sd_path = root / "policy_config.json", root / "policy_state_dict.pt"
    if not cfg_path.is_file() or not sd_path.is_file():
        raise FileNotFoundError(f"{checkpoint_dir} must contain policy_config.json and policy_state_dict.pt")
    payload = json.loads(cfg_path.read_text())
    if "vlm_model_name" not in payload:
        raise ValueError("legacy FastVLMPolicy checkpoints (nested backbone config) are not supported by the HIP path")
    config = FastVLAConfig(**payload)
    state = torch.load(sd_path, map_location="cpu")
    chunk = read_extras(root).get("action_chunk") or {}
    check_head_width(state, config.action_dim, chunk, root, read_extras(root).get("action_head"))
    head_kw = strata_need_draws(flow_kwargs(read_extras(root).get("action_head")))
    # the file decides: no record means the record's defaults (1, 1, "mse", 1.0), whatever the environment twins say -- a plain checkpoint loads as a plain policy
    policy = FastVLAPolicy(config, chunk_size=int(chunk.get("chunk_size", 1)), n_action_steps=int(chunk.get("n_action_steps", 1)),
                           action_loss=chunk.get("loss", "mse"), action_loss_beta=float(chunk.get("beta", 1.0)),
                           temporal_ensemble_coeff=chunk.get("temporal_ensemble_coeff", False), action_dim_weights=chunk.get("dim_weights", False),
                           action_step_weights=chunk.get("step_weights", False),      # (False: off, whatever the twin says)
                           **head_kw, **prefix_kwargs(read_extras(root).get("action_head")))
    check_fusion_width(state, policy, root)
    check_action_head_shape(state, policy, root)
    vlm = {k[len(BACKBONE_PREFIX):]: v for k, v in state.items() if k.startswith(BACKBONE_PREFIX)}
    if vlm:
        policy.model.backbone.load_backbone_state(vlm)
    own = [k for k in policy.state_dict() if not any(m in k for m in EXTRA_STATE_MARKS)]
    missing = [k for k in own if k not in state]
    if missing:
        raise KeyError(f"checkpoint lacks head tensors: {missing}")
    extra = {k: v for k, v in state.items() if any(m in k for m in EXTRA_STATE_MARKS)}   # folded dataset statistics travel with the state dict (round-5 files: the splice mode too)
    policy.load_state_dict({**{k: state[k] for k in own}, **extra})
    ex = read_extras(root)
    if "splice_image_tokens" in ex:
        policy.model.backbone.splice_image_tokens = bool(ex["splice_image_tokens"])
    if ex.get("lora"):
        load_lora_adapters(policy, root, ex["lora"])
    policy.eval()
    return policy


def flow_kwargs(rec) -> dict:
    """FastVLAPolicy's action-head arguments from a checkpoint's "action_head" record; no record: the regression head, whatever the twins say"""
    if rec and rec.get("type") == "bins":      # (the file decides here too: every action_bins_* argument is explicit, so no twin is read)
        return {"action_head": "bins", "action_bins": int(rec["bins"]), "action_bins_range": [tuple(float(x) for x in p) for p in rec["range"]],
                "action_bins_sigma": float(rec.get("sigma", 0.0)), "action_bins_decode": str(rec.get("decode", "argmax"))}
    if not rec or rec.get("type") != "flow":
        return {"action_head": "regression"}
    # the embedding's periods and the time distribution's parameters are constants of this build: a record written with others would load into another network
    from ..fastvla.modeling_fastvla import FLOW_DIST_A, FLOW_DIST_B, FLOW_MAX_PERIOD, FLOW_MIN_PERIOD
    ours = {"min_period": FLOW_MIN_PERIOD, "max_period": FLOW_MAX_PERIOD, "dist_a": FLOW_DIST_A, "dist_b": FLOW_DIST_B}
    theirs = {k: float(rec.get(k, v)) for k, v in ours.items()}
    if theirs != ours:
        raise ValueError(f"the checkpoint's action_head record was written with {theirs}, this build's flow head uses {ours}: the time embedding / time "
                         "distribution would differ from the one the weights were trained with")
    kw = {"action_head": "flow", "flow_steps": int(rec.get("steps", 10)), "flow_time_dim": int(rec["time_dim"]), "flow_time_dist": rec.get("time_dist", "uniform"),
          "flow_seed": rec.get("seed")}
    if rec.get("time_range"):      # ("time_dist" may be "beta:1.5,1.0"; these two are written only when set: a record without them maps to what it mapped to)
        kw["flow_time_range"] = tuple(float(x) for x in rec["time_range"])
    if rec.get("time_stratify"):
        kw["flow_time_stratify"] = True
    if rec.get("solver"):      # (written only when it is not Euler: an Euler run's record, and what it maps to, is what it was)
        kw["flow_solver"] = str(rec["solver"])
    return kw


def strata_need_draws(kw: dict) -> dict:
    """flow_kwargs' result for a LOAD: the strata are dealt to the draws of a training step, and the number of draws is a property of the run that no checkpoint
    records -- a load without FASTVLA_FLOW_NOISE_DRAWS > 1 (inference, say) gets the recorded distribution without strata (False: off, whatever the twin says); a
    resumed Trainer builds its policy from the run's own options"""
    if kw.get("flow_time_stratify"):
        from ..fastvla.options import resolve_flow_noise_draws
        if resolve_flow_noise_draws(None, action_head="flow") == 1:
            kw = {**kw, "flow_time_stratify": False}
    return kw


def prefix_kwargs(rec) -> dict:
    """FastVLAPolicy's action-prefix arguments from a checkpoint's "action_head" record.  The file decides: no "prefix_max_delay" means a head without the
    mask columns, whatever the FASTVLA_FLOW_PREFIX_MAX_DELAY twin says"""
    if not rec or rec.get("type") != "flow" or not rec.get("prefix_max_delay"):
        return {"flow_prefix_max_delay": False}
    return {"flow_prefix_max_delay": int(rec["prefix_max_delay"]), "flow_prefix_delay_dist": rec.get("prefix_delay_dist", "uniform"),
            "flow_prefix_delay_rate": float(rec.get("prefix_delay_rate", 0.5))}


def load_lora_adapters(policy: FastVLAPolicy, checkpoint_dir, lora_extras: dict, optim: dict | None = None) -> None:
    """Put the policy into LoRA mode as hip_extras.json records it and load the adapter file it names.  Raises when the file (or a tensor in it) is missing:
    running the base model in place of the fine-tuned one silently is the one thing this must not do.  optim: the parameter-group options of the run being
    resumed (optimizer.pt's record; Trainer passes it): used when THIS call is what switches LoRA mode on and no FASTVLA_* twin asks for others."""
    f = Path(checkpoint_dir) / lora_extras.get("file", LORA_FILE)
    if not f.is_file():
        raise FileNotFoundError(f"{Path(checkpoint_dir) / EXTRAS_FILE} records LoRA adapters (rank {lora_extras.get('rank')}) in '{f.name}', which is not there")
    # (a policy that is already in LoRA mode keeps the backward mode it was started in and just receives the adapters)
    mode = {} if getattr(policy, "_unfrozen", None) is not None else {"lora_direct": bool(lora_extras.get("direct", False))}
    if optim and getattr(policy, "_unfrozen", None) is None:
        from fastvla_hip import optim as _optim
        if not _optim.options_from_env():
            mode.update(_optim.explicit_kwargs(optim))
    un = policy.enable_backbone_training(lora_rank=int(lora_extras["rank"]), lora_alpha=float(lora_extras["alpha"]), lora_targets=list(lora_extras["targets"]),
                                         lora_dora=bool(lora_extras.get("dora")), lora_rslora=bool(lora_extras.get("rslora")), **mode)
    un.load_lora_state(torch.load(f, map_location="cpu"))


def save_policy_checkpoint(policy: FastVLAPolicy, checkpoint_dir: str, include_backbone: bool = False) -> Path:
    """policy_config.json + policy_state_dict.pt under the reference's key names (trainer.py:246-255).  include_backbone=True adds
    the VLM tensors the engine was packed from as `model.backbone.model.<canonical key>` and the tied `lm_head.weight`, which is what
    makes the file loadable by the reference's strict `load_state_dict`."""
    d = Path(checkpoint_dir)
    d.mkdir(parents=True, exist_ok=True)
    (d / "policy_config.json").write_text(json.dumps(dataclasses.asdict(policy.config), indent=2))
    # (the splice mode goes to the side file: policy_state_dict.pt keeps the reference's keys only, + `io_norm.*` while dataset statistics are folded)
    state = {k: v.detach().cpu().clone() for k, v in policy.state_dict().items() if SPLICE_KEY_MARK not in k}
    un = getattr(policy, "_unfrozen", None)
    extras = {"splice_image_tokens": bool(policy.model.backbone.splice_image_tokens), "train_backbone": un is not None,
              "train_tower": bool(un is not None and un.train_tower)}
    lora_cfg = getattr(un, "lora", None)
    if lora_cfg is not None:
        if un.lora_merged and not include_backbone:
            raise ValueError("merge_lora() changed the decoder master: save with include_backbone=True (adapters alone no longer describe the model)")
        if not un.lora_adapters_zero:      # (right after merge_lora() the adapters are zero and the master holds everything: a plain checkpoint)
            torch.save(un.lora_state(), d / LORA_FILE)
            extras["lora"] = {**lora_cfg, "file": LORA_FILE}
            if getattr(un, "lora_direct", False):      # (written only when on: a missing key means the projected backward, and a projected run's file is what it was)
                extras["lora"]["direct"] = True
        elif (d / LORA_FILE).is_file():
            (d / LORA_FILE).unlink()
    aug = policy.model.backbone.augmentation_record()
    if aug is not None:      # (written only when on) the run's image augmentation: its options and seed; the batch counter travels in optimizer.pt
        extras["augment"] = {"options": aug["options"], "seed": aug["seed"]}
    rec = policy.model.chunk_record(getattr(policy, "n_action_steps", 1), getattr(policy, "temporal_ensemble_coeff", None)) if hasattr(policy.model, "chunk_record") else None
    if rec is not None:      # (written only when something differs from the defaults)
        extras["action_chunk"] = rec
    frec = policy.model.flow_record() if hasattr(policy.model, "flow_record") else None
    if frec is not None:     # (written only in flow mode)
        extras["action_head"] = frec
    if any(extras.values()):
        (d / EXTRAS_FILE).write_text(json.dumps(extras, indent=2))
    if include_backbone:
        embed = None
        for name, t in policy.model.backbone.source_tensors():
            state[BACKBONE_PREFIX + name] = t.detach().cpu()
            if name == "model.embed_tokens.weight":
                embed = state[BACKBONE_PREFIX + name]
        if embed is not None and BACKBONE_PREFIX + "lm_head.weight" not in state:
            state[BACKBONE_PREFIX + "lm_head.weight"] = embed    # tied embeddings: the HF state dict lists both names
    torch.save(state, d / "policy_state_dict.pt")
    return d
