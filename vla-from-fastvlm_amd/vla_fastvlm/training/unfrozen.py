"""Unfrozen-backbone training on the HIP path: decoder + mm_projector + action expert trainable, FastViT-HD
tower frozen, image tokens spliced in front of the text.

The reference exposes `freeze_backbone` (fastvla/configuration_fastvla.py:23, applied at model/fastvlm_adapter.py:170-173) but wraps the
backbone forward in an unconditional `@torch.no_grad()` (model/fastvlm_adapter.py:501), so its own loop (training/trainer.py:171-182)
only ever trains the head.  Because of that, `freeze_backbone=False` ALONE keeps the reference's behaviour here too (frozen backbone, head
training); the VLM is fine-tuned only after an explicit `policy.enable_backbone_training()` (or FASTVLA_TRAIN_BACKBONE=1 together with
`freeze_backbone=False`).  The step body is the reference's -- loss -> backward -> clip_grad_norm_(1.0) over ALL parameters -> AdamW ->
schedule -- with every kernel in libfastvla_hip.so (fv_train_forward_backward, fv_adamw_clip_step, fv_train_commit).

All trainable tensors live in ONE flat fp32 buffer (fv_train_layout: [head | projector | embedding | layers | final norm], matrices in the
library's packed layout); gradients, Adam's m and v mirror it.  Under torch.distributed the gradient is exchanged per BUCKET while the
backward pass is still running (training/dp.py BucketedGradExchange, driven by the library's fv_bucket_cb).

LoRA mode (`lora={"rank", "alpha", "targets"}`; fv_train_lora_*): the decoder's matrices stay FROZEN in that master and every target matrix runs as
W0 + (alpha / rank) B A; action expert and mm_projector still train in full.  The trainable tensors then live in a second, small flat buffer
(fv_train_lora_layout: [head | projector | layer adapters]) and the gradient that is exchanged, Adam's m / v and the optimiser step cover THAT buffer only:
forward/backward (unchanged, full dW') -> fv_train_lora_project -> ONE all-reduce -> clip + AdamW -> fv_train_lora_commit.  The full-size m / v are never
allocated; the full master and the full gradient buffer remain.

Direct LoRA mode (`lora_direct=True`; fv_train_lora_forward_backward): the backward writes head, projector and adapter gradients straight into the
trainable-layout gradient buffer (dA = s (dY B)^T X, dB = s dY^T (X A^T) from the gradient rows and the kept activations) -- the full weight gradient is never
formed, the full-size gradient buffer is never allocated (`self.g is None`) and fv_train_lora_project is not called; everything behind the backward is the same.

Variants (keys of `lora`, present only when true): "rslora" -- s = alpha / sqrt(rank); "dora" -- every target also trains a magnitude per output row,
W' = diag(m / ||V||_row) V over V = W0 + s B A (the norm a constant in the backward, as in PEFT).  m starts as the row norms (fv_train_lora_init_magnitude), so
the adapted model starts as the base model bit for bit; the step is the projected one (the commit refreshes the norms the projection reads); not with lora_direct.

Parameter groups (`optim={"lr_scales", "no_decay", "layer_decay", "lora_plus_ratio", "freeze"}`, fastvla_hip/optim.py): with one of them set the optimiser step is
fv_adamw_clip_step_groups over a table built from the trainable buffer's layout -- a learning-rate factor, a weight decay and a frozen flag per group, ONE clip
norm over the non-frozen elements -- and the step also returns every group's gradient norm.  With none set the step is fv_adamw_clip_step, as before.

Step guard (policy.enable_step_guard(); fastvla/guard_state.py): the optimiser call of any kind becomes fv_adamw_clip_step_guarded -- a step whose gradient is
non-finite or whose backward clamped an fp16 operand is skipped on the device, the loss scale backs off and grows again there -- and the 50-step host poll of
the saturation counter below is not run.  The commit after a skipped step still runs: it rebuilds the same operand images.

EMA (policy.enable_ema(); fastvla/ema_state.py): the optimiser call of either kind becomes fv_adamw_clip_step_ema, which also moves an average of `trainable`
in the same pass; with it off the calls are the ones above.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from fastvla_hip import HEAD_KEYS

from .dp import BucketedGradExchange, GradExchange


class UnfrozenState:
    def __init__(self, policy, bucket_min_numel: int = 1 << 22, train_tower: bool = False, lora: Optional[Dict] = None, lora_seed: int = 0,
                 lora_direct: bool = False, optim: Optional[Dict] = None):
        from fastvla_hip import optim as _optim
        self.optim = _optim.normalize_options(**(optim or {}))     # {} = the single-group step; what optimizer.pt records and a resume compares
        if "lora_plus_ratio" in self.optim and lora is None:
            raise ValueError("lora_plus_ratio needs LoRA adapters (lora_rank)")
        self._group_table: Optional[tuple] = None                  # (weight decay, device table): built on the first step that uses it
        self.group_names: Optional[List[str]] = None
        self.group_norms: Optional[torch.Tensor] = None
        m = policy.model
        bb = m.backbone
        self.policy = policy
        eng = bb.engine()
        if eng.llm_precision != 1:
            raise RuntimeError("backbone training needs the split-bf16 decoder policy (llm_precision=1): its bf16 weight copies are refreshed "
                               f"from the fp32 master after every step; this engine runs llm_precision={eng.llm_precision}")
        if lora is not None and train_tower:
            raise ValueError("LoRA adapters go with a frozen vision tower: lora and train_tower cannot be combined")
        if lora_direct and lora is None:
            raise ValueError("lora_direct needs a LoRA configuration (lora_rank)")
        if lora_direct and lora.get("dora"):
            raise ValueError("lora_dora and lora_direct cannot be combined: DoRA's magnitude gradient needs the full weight gradient (the projected backward)")
        eng.train_begin()
        self.train_tower = bool(train_tower)
        self.lora = dict(lora) if lora is not None else None      # {"rank", "alpha", "targets"}: the decoder's matrices frozen, adapters trained
        self.lora_direct = bool(lora_direct)                      # the run's backward mode: NOT part of self.lora (what adapter / optimiser files compare)
        if self.lora is not None:
            eng.train_lora_begin(self.lora["rank"], self.lora["alpha"], self.lora["targets"], dora=bool(self.lora.get("dora")), rslora=bool(self.lora.get("rslora")))
        if self.train_tower:
            eng.train_tower_begin()        # the FastViT-HD tower's inference-form tensors join the flat master (fv_train_tower_*)
        self._tws: Dict[int, torch.Tensor] = {}
        self._dto: Dict[int, torch.Tensor] = {}
        self.eng = eng
        self.tensors, self.total, self.n_buckets = eng.train_layout()
        dev = eng.device
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=dev)
        eng.train_export_params(self.flat)
        # the 12 head tensors move into the front of the flat buffer and the nn.Parameters are re-pointed at it, so state_dict(), a torch
        # optimiser or LeRobot's checkpointing keep seeing the live values
        old = m.materialize(dev)
        hn = eng.head_numel()
        self.flat[:hn].copy_(old)
        self.lflat: Optional[torch.Tensor] = None
        self.lora_merged, self.lora_adapters_zero = False, False
        if self.lora is not None:
            # the trainable buffer: its head | projector front starts as the master's (the two share their offsets), lora_A as PEFT initialises it, lora_B = 0
            from fastvla_hip import lora as _lora
            self.lora_tensors, self.lora_total = eng.train_lora_layout()
            self.front = next(t["offset"] for t in self.lora_tensors if ".lora_" in t["name"])
            self.lflat = torch.zeros(self.lora_total, dtype=torch.float32, device=dev)
            self.lflat[: self.front].copy_(self.flat[: self.front])
            _lora.init_adapters(self.lflat, self.lora_tensors, seed=lora_seed)
            if self.lora.get("dora"):
                eng.train_lora_init_magnitude(self.flat, self.lflat)      # m = ||W0|| per row (lora_B = 0): m / n == 1 exactly
                eng.train_lora_commit(self.flat, self.lflat)              # the projection reads the norms and the master of a commit: the same operand images, bit for bit
            self.lg = torch.zeros_like(self.lflat)
        self.trainable = self.lflat if self.lora is not None else self.flat     # what the optimiser steps over
        views = eng.head_views(self.trainable[:hn])
        with torch.no_grad():
            for p, k in zip(m.head_parameters(), HEAD_KEYS):
                p.data = views[k]
        m._flat = self.trainable[:hn]
        self.g = None if self.lora_direct else torch.zeros_like(self.flat)      # direct LoRA: the full-size gradient buffer does not exist
        self.acc: Optional[torch.Tensor] = None
        self.m, self.v = torch.zeros_like(self.trainable), torch.zeros_like(self.trainable)
        self.step_count, self.micro = 0, 0
        self.norm = torch.zeros(1, device=dev)
        self.loss_scale_log2 = 12
        self.saturation_check_every = 50
        self.bucketed = BucketedGradExchange(dev, min_numel=bucket_min_numel)
        self.whole = GradExchange(dev)
        self._ws: Dict[tuple, torch.Tensor] = {}
        bb.splice_image_tokens = True          # the model being trained IS the spliced one: inference must run the same graph
        bb._trained_tensors = self.named_backbone_tensors   # checkpoint export reads the master, not the original weight source
        pending = policy._opt_state if isinstance(policy._opt_state, dict) and "resume" in policy._opt_state else None
        policy._opt_state = {"m": self.m, "v": self.v, "step": 0, "flat": self.trainable, "norm": self.norm}
        if pending is not None and pending["resume"]["m"].numel() == self.m.numel():   # load_optimizer_state() ran before this state existed
            r = pending["resume"]
            self.m.copy_(r["m"].to(dev))
            self.v.copy_(r["v"].to(dev))
            self.step_count = int(r["step"])
            policy._opt_state["step"] = self.step_count

    # ------------------------------------------------------------------ parameter groups
    def optim_kwargs(self) -> Dict:
        """the options as enable_backbone_training's keywords, every one explicit (an unset one as its empty value, so no environment twin fills it in)"""
        from fastvla_hip import optim as _optim
        return _optim.explicit_kwargs(self.optim)

    def param_groups(self, weight_decay: float):
        """-> (groups, names) of the trainable buffer under this run's options (fastvla_hip.optim.build_param_groups over its layout)"""
        from fastvla_hip import optim as _optim
        tensors = self.lora_tensors if self.lora is not None else self.tensors
        return _optim.build_param_groups(tensors, weight_decay=weight_decay, total=self.trainable.numel(), **self.optim)

    def _groups_for(self, weight_decay: float):
        """the device table for this weight decay.  The table carries the groups' decays as absolute values, so it is built on the first step and REBUILT when a
        later step passes another decay -- a configuration call each time (fv_adamw_groups_destroy / _create: they allocate and synchronise the device).  With a
        constant decay, which is what Trainer passes, the step allocates nothing and reads nothing back; a loop that schedules the decay pays a synchronisation
        per change."""
        key = float(weight_decay)
        if self._group_table is None or self._group_table[0] != key:
            if self._group_table is not None:
                self._group_table[1].close()
            groups, names = self.param_groups(key)
            self._group_table = (key, self.eng.adamw_groups(groups, self.trainable.numel()))
            self.group_names, self.group_norms = names, torch.zeros(len(groups), device=self.eng.device)
        return self._group_table[1]

    # ------------------------------------------------------------------ views / export
    def named_backbone_tensors(self) -> Dict[str, torch.Tensor]:
        """canonical checkpoint key -> fp32 copy of every trained decoder / projector tensor (q / k / v and gate / up unpacked)"""
        out = {k: v for k, v in self.eng.train_named_tensors(self.flat).items() if not k.startswith("head.")}
        # a trained tower lives in the master in its inference form (every ConvFFN's BatchNorm folded into its 7x7): written back under the
        # checkpoint's own keys as that conv + an identity BatchNorm, which is what a loader (this build's or the reference's) folds to the same tensor
        bn_eps = float(self.eng.model.tower.bn_eps)
        for k in [k for k in out if k.endswith(".convffn.conv.folded.weight")]:
            pre = k[: -len("folded.weight")]
            w = out.pop(k)
            c = w.shape[0]
            out[pre + "conv.weight"] = w
            out[pre + "bn.weight"] = torch.ones(c, device=w.device)
            out[pre + "bn.bias"] = out.pop(pre + "folded.bias")
            out[pre + "bn.running_mean"] = torch.zeros(c, device=w.device)
            out[pre + "bn.running_var"] = torch.full((c,), 1.0 - bn_eps, device=w.device)
        return out

    # ------------------------------------------------------------------ LoRA: adapters in and out, merge
    def lora_state(self) -> Dict:
        """what an adapter checkpoint holds: {"config": {rank, alpha, targets[, dora][, rslora]}, "tensors": {PEFT name -> lora_A / lora_B (DoRA:
        lora_magnitude_vector too), and the mm_projector's four tensors, which train in full beside them}} (CPU copies)"""
        assert self.lora is not None
        out = {}
        for t in self.lora_tensors:
            if t["bucket"] == 0:
                continue
            v = self.lflat[t["offset"]: t["offset"] + t["numel"]]
            out[t["name"]] = (v.view(t["rows"], t["cols"]) if t["rows"] > 1 else v).detach().cpu().clone()
        return {"config": dict(self.lora), "tensors": out}

    def load_lora_state(self, state: Dict) -> None:
        """the inverse: every adapter (and projector tensor) of this layout must be in `state["tensors"]` with its shape -- a missing one raises"""
        assert self.lora is not None
        cfg = state.get("config", {})
        if int(cfg.get("rank", -1)) != self.lora["rank"] or list(cfg.get("targets", [])) != list(self.lora["targets"]) or float(cfg.get("alpha", -1)) != float(self.lora["alpha"]):
            raise ValueError(f"adapter file was written with {cfg}, this run uses {self.lora}")
        if any(bool(cfg.get(k)) != bool(self.lora.get(k)) for k in ("dora", "rslora")):     # (a file that predates the keys is plain LoRA)
            raise ValueError(f"adapter file was written with {cfg}, this run uses {self.lora} (DoRA / rsLoRA adapters and plain LoRA adapters are not interchangeable)")
        tensors = state.get("tensors", {})
        want = [t for t in self.lora_tensors if t["bucket"] != 0]
        missing = [t["name"] for t in want if t["name"] not in tensors]
        if missing:
            raise KeyError(f"adapter file lacks {len(missing)} tensors, e.g. {missing[:3]}")
        for t in want:
            src = tensors[t["name"]]
            if src.numel() != t["numel"]:
                raise ValueError(f"{t['name']}: {tuple(src.shape)} in the file, {t['rows']} x {t['cols']} expected")
            self.lflat[t["offset"]: t["offset"] + t["numel"]].copy_(src.reshape(-1).to(self.lflat.device, torch.float32))
        self.lora_adapters_zero = False
        self.commit()

    def commit(self) -> None:
        """operand images <- the current parameters (fv_train_commit / fv_train_lora_commit), and every cache computed with the old ones dropped"""
        if self.lora is not None:
            self.eng.train_lora_commit(self.flat, self.lflat)
        else:
            self.eng.train_commit(self.flat)
        bb = self.policy.model.backbone
        bb.clear_prefix_cache()
        bb.clear_prompt_cache()

    def merge_lora(self) -> None:
        """W0 += s B A into the master (fv_train_lora_merge: the very fp32 values the adapted commit rounds), then lora_B = 0: the model is unchanged, the master
        is now a plain fine-tuned decoder that named_backbone_tensors() / the backbone export write under the reference's keys.  DoRA: the master receives
        diag(m / n) (W0 + s B A), and the magnitudes are re-initialised from it (m = its row norms, m / n == 1 exactly), so the adapted commit of the merged
        master is the plain one."""
        assert self.lora is not None
        self.policy._ema_refuse_in_scope("merge_lora()")
        self.eng.train_lora_merge(self.flat, self.lflat)
        dora = bool(self.lora.get("dora"))
        for t in self.lora_tensors:
            if t["name"].endswith(".lora_B.weight") or (dora and t["name"].endswith(".lora_magnitude_vector.weight")):
                self.lflat[t["offset"]: t["offset"] + t["numel"]].zero_()
                self.m[t["offset"]: t["offset"] + t["numel"]].zero_()
                self.v[t["offset"]: t["offset"] + t["numel"]].zero_()
        if dora:
            self.eng.train_lora_init_magnitude(self.flat, self.lflat)
        self.lora_merged, self.lora_adapters_zero = True, True
        self.commit()

    def _workspace(self, B: int, T: int) -> torch.Tensor:
        key = (B, T)
        if key not in self._ws:
            self._ws.clear()                   # one shape at a time: the stash is ~0.5 GB per sample at FastVLM-0.5B
            self._ws[key] = self.eng.train_workspace(B, T)
        return self._ws[key]

    # ------------------------------------------------------------------ one step
    def prepare(self, batch: Dict) -> Dict:
        """everything that does not depend on the trainable parameters: image prep + the FROZEN tower, tokenisation"""
        pol, bb, eng = self.policy, self.policy.model.backbone, self.eng
        dev = eng.device
        images = pol.processor.prepare_images(batch["images"], dev, augment=pol.training)     # (image augmentation, when on: training batches only)
        states = pol.processor.prepare_states(batch["states"], dev).float()
        tasks = pol.processor.prepare_tasks(batch["tasks"], batch_size=images.shape[0])
        targets, pad = pol.model.chunk_targets(batch["actions"].to(dev, torch.float32), batch.get("action_is_pad"))
        pix = bb._prepare_images_tensor(images, dev, augment=pol.training)
        tower_out = None
        if not self.train_tower:           # a trainable tower's forward depends on the parameters: it belongs to step()
            with torch.no_grad():
                _, tower_out = eng.vision_forward(pix, return_tower_out=True)
        text = bb._prep_text(tasks, dev)
        ids, mask = text["input_ids"], text["attention_mask"]
        T = ids.shape[1]
        Tp = (T + 7) // 8 * 8                  # the training kernels want whole 16-byte rows of ids: right-pad, masked
        if Tp != T:
            ids = torch.nn.functional.pad(ids, (0, Tp - T))
            mask = torch.nn.functional.pad(mask, (0, Tp - T))
        prep = {"tower_out": tower_out, "pix": pix if self.train_tower else None, "ids": ids, "lens": mask.to(torch.int32).sum(1).to(torch.int32), "states": states,
                "targets": targets.contiguous()}
        if pad is not None:      # (B, K) bool: set on the handle only around this batch's own step (a look-ahead prepare leaves the step in flight alone)
            prep["pad"] = pad.to(dev)
        return prep

    def step(self, batch: Optional[Dict] = None, *, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 1e-4,
             max_grad_norm: Optional[float] = 1.0, process_group=None, prepared: Optional[Dict] = None, grad_accum_steps: int = 1,
             force_sync: bool = False) -> Dict[str, torch.Tensor]:
        pol, eng = self.policy, self.eng
        pol._ema_refuse_in_scope("a training step")
        prep = prepared if prepared is not None else self.prepare(batch)
        B, T = prep["ids"].shape
        ws = self._workspace(B, T)
        k = max(1, int(grad_accum_steps))
        self.micro += 1
        sync = force_sync or self.micro % k == 0
        p = float(pol.config.dropout) if pol.training else 0.0
        m = pol.model
        m._drop_calls += 1
        # flow head: the library noises the targets from the step's (seed, offset) -- the policy's flow stream, a function of the optimiser step (a resumed
        # run continues it), which then serves the dropout mask too (another Philox key); otherwise the dropout stream as ever
        seed, offset = m.flow_train_draw(self.step_count, self.micro) if m.flow is not None and pol.training else \
            (m.flow_eval_draw() if m.flow is not None else (m._drop_seed, m._drop_calls))
        # per-bucket all-reduce under the backward pass; with accumulation the sum is exchanged once -- and in LoRA mode what is exchanged does not exist
        # before the projection has run: one all-reduce of the (small) trainable buffer
        overlap = k == 1 and sync and self.lora is None
        if overlap:
            self.bucketed.group = process_group
            self.bucketed.begin(self.g)
        # the step guard (policy.enable_step_guard(); fastvla/guard_state.py): None with it off -- every call below is then the one it was.  On: bound to the
        # backward (every gradient carries the loss scale times the guard's delta), observed after every micro-batch, consumed by the guarded step
        guard = pol._step_guard_attach(eng, self.loss_scale_log2)
        tower_out, tws, dto = prep["tower_out"], None, None
        if self.train_tower:
            if B not in self._tws:
                self._tws.clear(); self._dto.clear()
                self._tws[B] = eng.train_tower_workspace(B)
                t = eng.model.tower
                self._dto[B] = torch.zeros(B, t.num_tokens, t.out_dim, dtype=torch.float16, device=eng.device)
            tws, dto = self._tws[B], self._dto[B]
            eng.train_set_tower_grad(dto)
            tower_out = eng.train_tower_forward(prep["pix"], tws)
        if self.lora_direct:
            actions, loss, _ = eng.train_lora_forward_backward(self.flat, self.lflat, tower_out, prep["ids"], prep["lens"], prep["states"], prep["targets"], ws,
                                                               training=pol.training, dropout_p=p, seed=seed, offset=offset, lora_grads=self.lg, pad=prep.get("pad"))
        else:
            actions, loss, _ = eng.train_forward_backward(self.flat, tower_out, prep["ids"], prep["lens"], prep["states"], prep["targets"], ws,
                                                          training=pol.training, dropout_p=p, seed=seed, offset=offset, flat_grads=self.g,
                                                          bucket_cb=self.bucketed.bucket_ready if overlap else None, pad=prep.get("pad"))
        if self.train_tower:
            eng.train_tower_backward(prep["pix"], dto, tws, self.g, bucket_cb=self.bucketed.bucket_ready if overlap else None)
        if guard is not None:
            guard.observe()      # did this micro-batch's backward clamp an fp16 operand?  (sticky over the accumulation window)
        total = self.g
        if self.lora is not None:
            if not self.lora_direct:
                eng.train_lora_project(self.g, self.lflat, self.lg)    # dA, dB of every adapted matrix; head / projector gradients copied
            total = self.lg
        if k > 1:
            if self.acc is None:
                self.acc = torch.zeros_like(self.trainable)
            if self.micro == 1:
                self.acc.copy_(total)
            else:
                eng.grad_accumulate(self.acc, total)
            total = self.acc
        met = eng.head_loss_metrics() if eng.loss_is_chunked(prep.get("pad")) else None
        out = {"loss": loss[0], "mse": met[0] if met is not None else loss[0].detach(), "actions": m._shape_actions(actions), "synced": sync, "next": None}
        if getattr(m, "bins", None) is not None:      # a binned head: the fraction of valid elements whose most likely bin is the target's
            out["accuracy"] = met[2]
        if sync:
            if overlap:
                scale = self.bucketed.finish(eng.device)
            else:
                self.whole.group = process_group
                scale = self.whole.start(total) / k
                self.whole.finish(eng.device)
            self.step_count += 1
            self.micro = 0
            scale /= eng.train_loss_scale()      # every gradient of fv_train_forward_backward carries the loss scale (2^12 by default)
            ema = pol._ema_step_args(self.step_count)      # {} with EMA off: the calls below are then the ones they were (fastvla/ema_state.py)
            if guard is not None:
                from fastvla_hip.guard import all_reduce_flag
                all_reduce_flag(guard.flag(), process_group)      # one rank's flag skips the step on every rank (a NaN / inf survives the gradient sum by itself)
                ema = {**ema, "guard": guard}
            if self.optim:       # parameter groups: lr / decay per group, frozen groups untouched, every group's norm (no host read: a device tensor)
                table = self._groups_for(weight_decay)
                eng.adamw_step(self.trainable, total, self.m, self.v, self.step_count, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                               max_grad_norm=max_grad_norm or 0.0, grad_scale=scale, grad_norm_out=self.norm, groups=table, group_norms_out=self.group_norms,
                               **ema)
            else:
                eng.adamw_step(self.trainable, total, self.m, self.v, self.step_count, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                               max_grad_norm=max_grad_norm or 0.0, grad_scale=scale, grad_norm_out=self.norm, **ema)
            self.lora_adapters_zero = False
            # bf16 operand copies (and their transposes) follow the master (LoRA: W0 + s B A); per-image decoder prefixes / per-prompt features computed with
            # the OLD weights must not serve an eval between steps
            self.commit()
            pol._opt_state["step"] = self.step_count
            if guard is None and self.step_count % self.saturation_check_every == 0:
                # the backward's fp16 operands carry the gradient x 2^loss_scale: a clamp means the scale is too large for this model / loss
                # -- say so and halve it (every 50 optimiser steps: the read synchronises)
                n = eng.fp16_saturations(reset=True)
                if n and self.loss_scale_log2 > 0:
                    import warnings
                    self.loss_scale_log2 -= 1
                    eng.train_set_options(loss_scale_log2=self.loss_scale_log2, keep=True)
                    warnings.warn(f"{n} fp16 gradient-operand groups saturated in the last {self.saturation_check_every} steps: loss scale lowered to 2^{self.loss_scale_log2}")
        if guard is not None:      # the last guarded step's decision and the scale the next backward runs with: device tensors, nothing is read back
            rep = guard.report()
            out["step_skipped"], out["loss_scale"] = rep[0], rep[1] * eng.train_loss_scale()
        out["grad_norm"] = self.norm[0]
        if self.optim and self.group_norms is not None:
            out["group_grad_norms"], out["group_names"] = self.group_norms, self.group_names     # one norm per group (a device tensor) and the groups' labels
        return out
