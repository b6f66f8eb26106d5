"""EMA of the trainable weights at policy level (fastvla_hip/ema.py has the options and the schedule; the average itself is kept by the fused optimiser
step, fv_adamw_clip_step_ema).

The SHADOW is one fp32 buffer shaped like the run's trainable buffer -- head-only: the flat head buffer (model._flat); unfrozen: UnfrozenState.trainable, the
whole master, or in LoRA mode head + projector + adapters (+ DoRA magnitudes) -- created as a bitwise copy of it.  In a LoRA run the average is therefore taken
over lora_A, lora_B (and the DoRA magnitude) SEPARATELY, as PEFT users do; that is not the average of the products B A.

`ema_weights()` does not copy anything: for the length of the scope the shadow takes the trainable buffer's PLACE -- the head parameters, the flat head buffer
and the unfrozen state's buffer are re-pointed at it and the operand images are committed from it (fv_train_commit(shadow) / fv_train_lora_commit(master,
shadow)) -- so every reader (forward, compute_loss, select_action, state_dict(), a checkpoint written inside) sees the averaged weights.  On exit the live
buffer takes its place back and is committed: the model computes bit for bit what it computed before."""
from __future__ import annotations

import contextlib
import warnings
from typing import Dict, Optional

import torch

from fastvla_hip import HEAD_KEYS
from fastvla_hip import ema as _ema


def check_resume_ema(recorded: Dict, current: Dict) -> None:
    """A resumed run must average the way the checkpointed one did: other EMA options raise, naming both."""
    recorded, current = _ema.normalize_options(**dict(recorded)), _ema.normalize_options(**dict(current))
    if recorded != current:
        raise ValueError(f"optimizer.pt was written by a run with the EMA options {recorded}, this run uses {current}: "
                         "resume with the checkpoint's options (enable_ema(decay, warmup, update_after) or their FASTVLA_EMA_* twins)")


class EmaMixin:
    """enable_ema / disable_ema / ema_weights / apply_ema for a policy with `.model` (FastVLMWithExpert) and, optionally, `._unfrozen` (UnfrozenState)"""

    _ema: Optional[Dict] = None          # {"options", "shadow", "live", "updates", "scope", "weight"} while EMA is on
    _ema_env_off: bool = False           # disable_ema() ran: the environment twin does not switch it back on

    # ------------------------------------------------------------------ on / off
    @property
    def ema_enabled(self) -> bool:
        return self._ema is not None

    @property
    def ema_shadow(self) -> Optional[torch.Tensor]:
        return self._ema["shadow"] if self._ema is not None else None

    def enable_ema(self, decay: Optional[float] = None, warmup: Optional[bool] = None, update_after: Optional[int] = None) -> Dict:
        """Keep an exponential moving average of the trainable weights, updated inside the optimiser step of every SYNCED micro-batch (accumulation micro-steps
        never touch it).  decay (default 0.999), warmup (default True: d_t = min(decay, (1 + tau) / (10 + tau))), update_after (default 0: that many
        optimiser updates during which the average just follows the live weights) -- an explicit argument beats its environment twin FASTVLA_EMA_DECAY /
        FASTVLA_EMA_WARMUP / FASTVLA_EMA_UPDATE_AFTER.  Works before or after enable_backbone_training(): the average is (re)started as a bitwise copy of the
        trainable buffer the moment that buffer exists.  A second call with the same options keeps the running average; other options raise RuntimeError
        (disable_ema() first).  -> the options."""
        opts = _ema.resolve_options(decay, warmup, update_after)
        if self._ema is not None:
            if self._ema["options"] != opts:
                raise RuntimeError(f"EMA is already running with {self._ema['options']}: disable_ema() before asking for {opts}")
            return dict(opts)
        self._ema = {"options": opts, "shadow": None, "live": None, "updates": 0, "scope": False, "weight": None}
        self._ema_env_off = False
        self._ema_attach()
        return dict(opts)

    def disable_ema(self) -> None:
        """drop the average (and its buffer); the FASTVLA_EMA_DECAY twin does not switch it back on for this policy"""
        if self._ema is not None and self._ema["scope"]:
            raise RuntimeError("disable_ema() inside ema_weights(): leave the scope first")
        self._ema = None
        self._ema_env_off = True

    def _ema_from_env(self) -> None:
        """FASTVLA_EMA_DECAY alone switches EMA on (read where a training step begins, in the style of FASTVLA_TRAIN_BACKBONE)"""
        if self._ema is None and not self._ema_env_off and _ema.options_from_env() is not None:
            self.enable_ema()

    # ------------------------------------------------------------------ the buffers
    def _ema_live(self) -> Optional[torch.Tensor]:
        """the run's trainable buffer, None while it does not exist yet (a head that has not been moved into its flat device buffer)"""
        un = getattr(self, "_unfrozen", None)
        return un.trainable if un is not None else self.model._flat

    def _ema_attach(self) -> Optional[torch.Tensor]:
        """-> the shadow of the CURRENT trainable buffer, (re)created as its bitwise copy when that buffer is new; None when EMA is off or no buffer exists"""
        st = self._ema
        if st is None:
            return None
        if st["scope"]:
            return st["shadow"]
        live = self._ema_live()
        if live is None or not live.is_cuda:
            return None
        if st["live"] is None or st["live"].data_ptr() != live.data_ptr() or st["live"].numel() != live.numel():
            st["shadow"], st["live"], st["updates"] = live.detach().clone(), live, 0
        return st["shadow"]

    def _ema_step_args(self, step: int) -> Dict:
        """adamw_step's ema= / ema_weight= for optimiser update `step` ({} with EMA off); counts the update"""
        if self._ema is None:
            return {}
        shadow = self._ema_attach()
        w = _ema.ema_weight(self._ema["options"], step)
        self._ema["updates"] += 1
        self._ema["weight"] = w
        return {"ema": shadow, "ema_weight": w}

    def _ema_refuse_in_scope(self, what: str) -> None:
        if self._ema is not None and self._ema["scope"]:
            raise RuntimeError(f"{what} inside ema_weights(): the averaged weights stand in for the live ones there -- leave the scope first")

    def _ema_place(self, buf: torch.Tensor) -> None:
        """make `buf` the buffer every reader takes for the trainable one"""
        m, un = self.model, getattr(self, "_unfrozen", None)
        if un is not None:
            if un.lora is not None:
                un.lflat = buf
            else:
                un.flat = buf
            un.trainable = buf
            eng, head = un.eng, buf[: un.eng.head_numel()]
        else:
            eng, head = m._engine(), buf
        views = eng.head_views(head)
        with torch.no_grad():
            for p, k in zip(m.head_parameters(), HEAD_KEYS):
                p.data = views[k]
        m._flat = head

    def _ema_commit(self) -> None:
        """operand images <- the buffer in place, every cache computed with other weights dropped"""
        un = getattr(self, "_unfrozen", None)
        if un is not None:
            un.commit()
        else:
            bb = self.model.backbone
            bb.clear_prefix_cache()
            bb.clear_prompt_cache()
        if hasattr(self, "_action_queue"):
            self._action_queue.clear()       # queued actions were predicted with the other weights

    # ------------------------------------------------------------------ evaluate / export
    @contextlib.contextmanager
    def ema_weights(self):
        """Every forward inside the scope (forward, compute_loss, select_action, select_action_chunk) uses the AVERAGED weights; a checkpoint written inside
        holds them.  Prefix and prompt caches are cleared on entry and on exit; on exit the live weights are committed back.  A nested entry is a no-op.
        Training steps and merge_lora() inside raise RuntimeError, and so does the scope itself with EMA off: a caller never evaluates live weights
        thinking they are averaged."""
        st = self._ema
        if st is None:
            raise RuntimeError("ema_weights(): EMA is off (enable_ema() or FASTVLA_EMA_DECAY)")
        if st["scope"]:
            yield self
            return
        shadow = self._ema_attach()
        if shadow is None:
            raise RuntimeError("ema_weights(): there is no average yet -- the trainable buffer does not exist before the first step on the device")
        live = st["live"]
        st["scope"] = True
        try:
            self._ema_place(shadow)
            self._ema_commit()
            yield self
        finally:
            self._ema_place(live)
            st["scope"] = False
            self._ema_commit()

    def apply_ema(self) -> None:
        """live trainable buffer <- the average, bitwise (Adam's m and v are kept), then commit: the export path.  apply_ema(); merge_lora() gives a plain
        fine-tuned decoder from the averaged adapters (the average of A and of B, not of B A)."""
        if self._ema is None:
            raise RuntimeError("apply_ema(): EMA is off (enable_ema() or FASTVLA_EMA_DECAY)")
        self._ema_refuse_in_scope("apply_ema()")
        shadow = self._ema_attach()
        if shadow is None:
            raise RuntimeError("apply_ema(): there is no average yet")
        self._ema["live"].copy_(shadow)
        un = getattr(self, "_unfrozen", None)
        if un is not None:
            un.lora_adapters_zero = False
        self._ema_commit()

    # ------------------------------------------------------------------ checkpoints
    def ema_record(self) -> Optional[Dict]:
        """what optimizer.pt holds under "ema" (None with EMA off): the options, the shadow (CPU) and the number of updates it has seen"""
        if self._ema is None or self._ema_attach() is None:
            return None
        return {"options": dict(self._ema["options"]), "shadow": self._ema["shadow"].detach().cpu().clone(), "updates": int(self._ema["updates"])}

    def load_ema_record(self, record: Optional[Dict]) -> None:
        """Called by a resume AFTER the live weights are restored.  A record into a run with EMA: the options must match (ValueError naming both), the shadow
        continues bit for bit.  A record into a run without EMA: a warning, the record is dropped.  No record into a run with EMA: the average starts from
        the restored live weights."""
        if record is not None and self._ema is None:
            warnings.warn(f"the checkpoint carries an EMA of the weights ({record.get('options')}), this run has EMA off: the average is dropped "
                          "(enable_ema() or FASTVLA_EMA_DECAY before resuming keeps it)")
            return
        if self._ema is None:
            return
        self._ema_refuse_in_scope("a resume")
        if record is not None:
            check_resume_ema(record["options"], self._ema["options"])
        self._ema["live"] = None            # (re)start from the restored live weights ...
        shadow = self._ema_attach()
        if record is not None and shadow is not None:
            src = record["shadow"]
            if src.numel() != shadow.numel():
                raise ValueError(f"the checkpointed EMA has {src.numel()} elements, this run's trainable buffer {shadow.numel()}")
            shadow.copy_(src.to(shadow.device))    # ... or continue the checkpointed average
            self._ema["updates"] = int(record.get("updates", 0))
