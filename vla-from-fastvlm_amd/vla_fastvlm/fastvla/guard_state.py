"""The guarded optimiser step at policy level (fastvla_hip/guard.py has the options and the device object; the decision itself is taken inside the fused step,
fv_adamw_clip_step_guarded).

With the guard on, every training route -- head-only, full decoder, tower, LoRA projected and direct, with or without parameter groups and EMA -- ends in the
guarded step: a non-finite gradient, or (backbone training) a backward whose fp16 operands saturated, leaves the weights, Adam's moments and the EMA shadow
untouched, and the loss scale backs off and grows again on the device.  Head-only training is fp32 and has no loss scale: its guard keeps delta = 1 and guards
against non-finite gradients only.  Off (the default), a run makes the calls it made and keeps every bit; no file gains a key.

The optimiser's `step` -- Adam's bias correction -- and the learning-rate schedule advance on a skipped step too: a rare skip shifts the bias correction by one
step, and a run without skips needs no second code path."""
from __future__ import annotations

import warnings
from typing import Dict, Optional

from fastvla_hip import guard as _guard


def check_resume_step_guard(recorded: Dict, current: Dict) -> None:
    """A resumed run must guard the way the checkpointed one did: other options raise, naming both."""
    recorded, current = _guard.normalize_options(**dict(recorded)), _guard.normalize_options(**dict(current))
    if recorded != current:
        raise ValueError(f"optimizer.pt was written by a run with the step guard options {recorded}, this run uses {current}: "
                         "resume with the checkpoint's options (enable_step_guard(...) or their FASTVLA_STEP_GUARD_* twins)")


class StepGuardMixin:
    """enable_step_guard / disable_step_guard / step_guard_stats for a policy with `.model` (FastVLMWithExpert) and, optionally, `._unfrozen` (UnfrozenState)"""

    _sg: Optional[Dict] = None          # {"options", "guard", "engine", "k", "pending"} while the guard is on
    _sg_env_off: bool = False           # disable_step_guard() ran: the environment twin does not switch it back on

    @property
    def step_guard_enabled(self) -> bool:
        return self._sg is not None

    def enable_step_guard(self, dynamic_loss_scale: Optional[bool] = None, growth_interval: Optional[int] = None, backoff_log2: Optional[int] = None,
                          growth_log2: Optional[int] = None, min_loss_scale_log2: Optional[int] = None, max_loss_scale_log2: Optional[int] = None) -> Dict:
        """Guard every later training step: skip it on the device when its gradient is non-finite or came from saturated fp16 operands, back the loss scale
        off by 2^backoff_log2 on a skip and grow it by 2^growth_log2 after growth_interval applied steps, inside [2^min_loss_scale_log2, 2^max_loss_scale_log2].
        dynamic_loss_scale=False pins the scale: the guard only skips.  An explicit argument beats its environment twin (FASTVLA_STEP_GUARD_GROWTH_INTERVAL and
        so on; FASTVLA_STEP_GUARD=1 alone switches the guard on).  Options are resolved and refused here, before any engine exists (ValueError naming both
        settings).  A second call with the same options keeps the running state; other options raise RuntimeError (disable_step_guard() first).  With the
        guard on the 50-step host poll of the saturation counter is not run, and the step's result gains "step_skipped" and "loss_scale", both device
        tensors.  -> the options."""
        opts = _guard.resolve_options(dynamic_loss_scale=dynamic_loss_scale, growth_interval=growth_interval, backoff_log2=backoff_log2, growth_log2=growth_log2,
                                      min_loss_scale_log2=min_loss_scale_log2, max_loss_scale_log2=max_loss_scale_log2)
        if self._sg is not None:
            if self._sg["options"] != opts:
                raise RuntimeError(f"the step guard is already running with {self._sg['options']}: disable_step_guard() before asking for {opts}")
            return dict(opts)
        un = getattr(self, "_unfrozen", None)
        if un is not None:
            _guard.guard_config(opts, un.loss_scale_log2)      # (refused here when the run's loss scale lies outside the bounds)
        self._sg = {"options": opts, "guard": None, "engine": None, "k": None, "pending": None}
        self._sg_env_off = False
        return dict(opts)

    def disable_step_guard(self) -> None:
        """drop the guard (unbound from the backward, its device state freed); the FASTVLA_STEP_GUARD twin does not switch it back on for this policy"""
        st, self._sg = self._sg, None
        self._sg_env_off = True
        if st is not None and st["guard"] is not None:
            self._sg_release(st)

    @staticmethod
    def _sg_release(st: Dict) -> None:
        eng, g = st["engine"], st["guard"]
        if getattr(eng, "h", None):
            if st["k"] is not None:
                eng.train_set_step_guard(None)
            g.close()
        st["guard"], st["engine"] = None, None

    def _step_guard_from_env(self) -> None:
        """FASTVLA_STEP_GUARD=1 switches the guard on (read where a training step begins, in the style of FASTVLA_EMA_DECAY)"""
        if self._sg is None and not self._sg_env_off and _guard.enabled_from_env():
            self.enable_step_guard()

    def _step_guard_attach(self, eng, loss_scale_log2: Optional[int]):
        """-> the StepGuard of this engine (None with the guard off), created -- and, for backbone training (loss_scale_log2 = the run's static exponent), bound
        to the backward -- on the first step that uses it: a configuration call, once.  A checkpointed state waiting for the guard is imported here."""
        st = self._sg
        if st is None:
            return None
        if st["guard"] is not None and (st["engine"] is not eng or st["k"] != loss_scale_log2 or not st["guard"]._h):
            st["pending"] = st["pending"] or (st["guard"].state() if st["guard"]._h and getattr(st["engine"], "h", None) else None)
            self._sg_release(st)
        if st["guard"] is None:
            g = _guard.StepGuard(eng, **_guard.guard_config(st["options"], loss_scale_log2))
            if loss_scale_log2 is not None:
                eng.train_set_step_guard(g)
            st["guard"], st["engine"], st["k"] = g, eng, loss_scale_log2
        if st["pending"] is not None:
            rec, st["pending"] = dict(st["pending"]), None
            rec["last_saturations"] = int(eng.fp16_saturations()) & 0xFFFFFFFF      # this engine's counter as it stands is not news to a restored guard
            st["guard"].load_state(rec)
        return st["guard"]

    def step_guard_stats(self) -> Dict:
        """The guard's counters and scale as plain numbers (a status call: it synchronises): delta_log2, good_steps, applied, skipped_nonfinite,
        skipped_saturated, saturated_applied, the last decision, and "loss_scale_log2" = the static exponent + delta_log2 (delta_log2 alone for head-only
        training).  Before the first guarded step: the initial state."""
        if self._sg is None:
            raise RuntimeError("step_guard_stats(): the step guard is off (enable_step_guard() or FASTVLA_STEP_GUARD=1)")
        st = self._sg
        if st["guard"] is not None:
            out = st["guard"].state()
        elif st["pending"] is not None:
            out = dict(st["pending"])
        else:
            out = {k: 0 for k in _guard.STATE_KEYS}
            out.update(last_apply=1, last_inv_delta=1.0, flag=0.0)
        un = getattr(self, "_unfrozen", None)
        out["loss_scale_log2"] = out["delta_log2"] + (un.loss_scale_log2 if un is not None else 0)
        return out

    # ------------------------------------------------------------------ checkpoints
    def step_guard_record(self) -> Optional[Dict]:
        """what optimizer.pt holds under "step_guard" (None with the guard off): the options and the guard's exported state (None before its first step)"""
        if self._sg is None:
            return None
        st = self._sg
        state = st["guard"].state() if st["guard"] is not None else (dict(st["pending"]) if st["pending"] is not None else None)
        return {"options": dict(st["options"]), "state": state}

    def load_step_guard_record(self, record: Optional[Dict]) -> None:
        """Called by a resume.  A record into a run with the guard: the options must match (ValueError naming both), the state continues bit for bit.  A record
        into a run without: a warning, the record is dropped.  No record into a run with the guard: it starts fresh."""
        if record is not None and self._sg is None:
            warnings.warn(f"the checkpoint carries a step guard's state ({record.get('options')}), this run has the guard off: the state is dropped "
                          "(enable_step_guard() or FASTVLA_STEP_GUARD=1 before resuming keeps it)")
            return
        if self._sg is None or record is None:
            return
        check_resume_step_guard(record["options"], self._sg["options"])
        if record.get("state") is not None:
            self._sg["pending"] = dict(record["state"])
