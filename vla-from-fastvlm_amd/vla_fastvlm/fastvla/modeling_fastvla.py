"""Standalone FastVLA policy (reference: src/vla_fastvlm/fastvla/modeling_fastvla.py:14-77): forward / compute_loss /
select_action / reset with the reference's signatures, plus `fused_train_step`, the native train step
(forward -> MSE -> head backward -> [all-reduce] -> clip -> AdamW in libfastvla_hip.so) that
vla_fastvlm.training.Trainer and bench.py drive."""
from __future__ import annotations

import os
from collections import deque
from typing import Dict, List, Optional

import torch
from torch import nn

from .configuration_fastvla import FastVLAConfig
from .ema_state import EmaMixin
from .fastvlm_with_expert import FastVLMWithExpert
from .flow_surface import FlowSurfaceMixin
from .guard_state import StepGuardMixin
from .options import (FLOW_DIST_A, FLOW_DIST_B, FLOW_MAX_PERIOD, FLOW_MIN_PERIOD, parse_weight_list, resolve_chunk_options,  # noqa: F401  (their public home)
                      resolve_flow_noise_draws, resolve_flow_options, resolve_flow_samples, resolve_flow_solver, resolve_policy_options,
                      resolve_prefix_options, resolve_rtc_options)
from .processor_fastvla import FastVLAProcessor


class FastVLAPolicy(nn.Module, EmaMixin, StepGuardMixin, FlowSurfaceMixin):
    config_class = FastVLAConfig
    name = "fastvla"

    def __init__(self, config: FastVLAConfig | None = None, chunk_size: Optional[int] = None, n_action_steps: Optional[int] = None,
                 action_loss: Optional[str] = None, action_loss_beta: Optional[float] = None, temporal_ensemble_coeff: Optional[float] = None,
                 action_dim_weights=None, action_step_weights=None, action_head: Optional[str] = None, flow_steps: Optional[int] = None,
                 flow_time_dim: Optional[int] = None, flow_time_dist: Optional[str] = None, flow_seed: Optional[int] = None, rtc: Optional[bool] = None,
                 flow_time_range=None, flow_time_stratify: Optional[bool] = None, rtc_schedule: Optional[str] = None, rtc_max_guidance_weight: Optional[float] = None, rtc_execution_horizon: Optional[int] = None,
                 flow_noise_draws: Optional[int] = None, flow_prefix_max_delay: Optional[int] = None, flow_prefix_delay_dist: Optional[str] = None,
                 flow_prefix_delay_rate: Optional[float] = None, rtc_method: Optional[str] = None, rtc_prefix_steps: Optional[int] = None,
                 flow_solver: Optional[str] = None, flow_samples: Optional[int] = None, flow_select: Optional[str] = None,
                 flow_coherence_decay: Optional[float] = None, action_bins: Optional[int] = None, action_bins_range=None, action_bins_sigma: Optional[float] = None,
                 action_bins_decode: Optional[str] = None) -> None:
        """Action chunks (an extension of this build, off by default; the core config is the reference's and has no field for them): chunk_size = K makes the
        head predict K future steps per observation -- forward / predict return (B, K, A), targets are (B, K, A) with an optional batch["action_is_pad"]
        (B, K) -- and select_action serves n_action_steps <= K of them from a queue before it runs the backbone again.  action_loss: "mse" | "l1" |
        "smooth_l1" (action_loss_beta), evaluated in the library as sum over non-padded elements / ALL B K A elements (LeRobot's convention).
        temporal_ensemble_coeff = c (ACT's temporal ensembling; needs n_action_steps == 1): select_action runs the backbone on EVERY call and returns the
        exponentially weighted mean (weights exp(-c i), i = 0 the oldest) of what the last K chunks predicted for this time step, kept on the device
        (fastvla_hip/ensemble.py).  action_dim_weights (A values) / action_step_weights (K values, or "discount:g" for g^k): weights of the loss per action
        dimension and per chunk step (set_action_loss_weights); a weight of 0 takes the element out like a padded step.
        Environment twins an explicit argument beats: FASTVLA_CHUNK_SIZE, FASTVLA_N_ACTION_STEPS, FASTVLA_ACTION_LOSS, FASTVLA_ACTION_LOSS_BETA,
        FASTVLA_TEMPORAL_ENSEMBLE_COEFF, FASTVLA_ACTION_DIM_WEIGHTS ("1,1,1,1,1,1,4"), FASTVLA_ACTION_STEP_WEIGHTS (a list, or "discount:0.98").

        action_head="flow" (default "regression"; FASTVLA_ACTION_HEAD): the flow-matching head (pi0 / SmolVLA convention, normalised action space).  The same
        12 tensors, fusion.0 reading K * A + flow_time_dim more columns; training noises the targets (x_t = t eps + (1 - t) a, t ~ flow_time_dist "uniform" |
        "logit_normal") and the configured loss, mask and weights compare the predicted velocity with u = eps - a; predict / select_action_chunk /
        select_action SAMPLE: flow_steps steps of the chosen solver from fresh noise (policy.flow_steps may be changed at any time), the queue and the temporal ensembling
        work on the sampled chunk as ever.  compute_loss / forward(batch) / the train step return the PREDICTED VELOCITY (normalised space) where the
        regression head returns actions.  In eval() mode the noise of a loss evaluation depends on the evaluation batch index only: two evaluations of the
        same weights give the same loss.  predict with autograd enabled on the head raises RuntimeError: sampling is not differentiated.  flow_seed: the noise
        streams' seed (default: torch's initial seed).  Twins: FASTVLA_FLOW_STEPS, FASTVLA_FLOW_TIME_DIM, FASTVLA_FLOW_TIME_DIST.  A policy that does not
        ask for flow calls nothing new.

        flow_time_dist="beta:<alpha>,<beta>" | "pi0" (flow head; FASTVLA_FLOW_TIME_DIST takes the same strings): the training time as pi0 and SmolVLA draw it --
        tau ~ Beta(alpha, beta), both in [0.25, 32]; "pi0" is "beta:1.5,1.0" on flow_time_range=(0.001, 1.0), which puts the mass on the noisy end and never
        reaches t = 0.  flow_time_range=(lo, hi) (FASTVLA_FLOW_TIME_RANGE="lo:hi"): t = lo + (hi - lo) tau for any distribution, 0 <= lo < hi <= 1.
        flow_time_stratify=True (FASTVLA_FLOW_TIME_STRATIFY; needs flow_noise_draws = S > 1): draw s of an observation takes the s-th of S equal-probability
        strata of tau, the cheapest variance reduction of an S-draw step.  All three go through ONE inverse CDF on the uniform the noising kernel already draws
        (fv_head_set_flow_time): eps, the prefix delay and the dropout stream do not move, and a policy that asks for none launches what it launched.  The bare
        word "beta" is a ValueError: a Beta without its parameters names no distribution.  hip_extras.json records the string under "time_dist", and
        "time_range" / "time_stratify" only when set; a resumed Trainer continues bit for bit.  flow_loss_per_time(batch, buckets) is the metric to judge a
        time distribution with.  ValueError, naming both settings and before any engine exists, for strata with one draw and for any of the three given
        explicitly with a regression head.

        flow_noise_draws=S (flow head, 1 .. 16, default 1; FASTVLA_FLOW_NOISE_DRAWS): S noise draws (t, eps) per observation wherever targets are noised --
        the train step on every route, compute_loss / forward(batch) in train() and in eval() mode (a smoother evaluation loss).  One step then computes the
        mean loss and the mean gradient of S single-draw steps (draw s draws what a single-draw step draws at offset + (s << 56)) for ONE backbone forward
        and backward: the head runs on S B rows, the backbone on B.  The returned velocity stays (B, K, A): draw 0.  A property of the run, like rtc: no
        checkpoint records it -- pass it again on resume, and the run continues bit for bit.  ValueError for S > 1 with a regression head.

        rtc=True (flow head, chunk_size > 1; FASTVLA_RTC): real-time chunking -- a re-plan is sampled GUIDED by the not-yet-executed rest of the previous chunk
        (fastvla_hip/rtc.py; fv_head_flow_sample_guided), so consecutive chunks stay in one mode of the distribution instead of jumping at the seam.
        select_action keeps its queue; when it runs dry the new chunk is guided by the last one read `shift` = the number of actions served since steps
        ahead, with inference delay 0; the first plan after reset() is unguided.  rtc_schedule "exp" | "linear" | "ones" | "zeros" (the prefix weights),
        rtc_max_guidance_weight (beta, default 5), rtc_execution_horizon (the last steps of the chunk left free, default n_action_steps); twins
        FASTVLA_RTC_SCHEDULE, FASTVLA_RTC_MAX_GUIDANCE_WEIGHT, FASTVLA_RTC_EXECUTION_HORIZON.  select_action_chunk(..., prev_chunk=, inference_delay=) is
        the explicit form for asynchronous callers.  A property of the run, not of the weights: no checkpoint records it, and a policy that does not
        ask for it calls nothing new.  Not with a regression head, chunk_size == 1 or temporal_ensemble_coeff (ValueError).

        flow_prefix_max_delay=D (flow head, 1 <= D < chunk_size; FASTVLA_FLOW_PREFIX_MAX_DELAY): action-prefix conditioning (Black, Ren, Equi, Levine 2025;
        fastvla_hip/prefix.py; fv_head_set_flow_prefix).  Training draws a delay d <= D per head row -- flow_prefix_delay_dist "uniform" | "exp" with
        flow_prefix_delay_rate (twins FASTVLA_FLOW_PREFIX_DELAY_DIST / _RATE) -- gives the first d steps of the chunk to the network clean and keeps them out
        of the loss, on every training route, in compute_loss / forward(batch) and with flow_noise_draws.  An ARCHITECTURE property, unlike rtc and
        flow_noise_draws: fusion.0.weight has chunk_size more columns, checkpoints record it, and a plain flow checkpoint does not load
        (fastvla_hip.prefix.widen_flow_state_dict turns one into a prefix head to fine-tune).  Not with a regression head, chunk_size == 1, D >= chunk_size
        or temporal_ensemble_coeff (ValueError).  rtc=True, rtc_method="prefix" (FASTVLA_RTC_METHOD; default "guidance"): a re-plan PINS its first
        min(rtc_prefix_steps, D, K - shift) steps to the last chunk read `shift` = the actions served since steps ahead and samples the rest with the plain
        three-launch sampler -- no guidance, no Jacobian, no beta; rtc_prefix_steps defaults to D (FASTVLA_RTC_PREFIX_STEPS).  The first plan after reset()
        pins nothing.  select_action_chunk(..., prev_chunk=, inference_delay=d) pins d <= D steps (ValueError above D).  rtc_schedule,
        rtc_max_guidance_weight and rtc_execution_horizon given together with "prefix" are refused.

        flow_solver="euler" | "midpoint" | "heun" | "rk4" (flow head; default "euler"; FASTVLA_FLOW_SOLVER): the integrator of EVERY sampling route -- predict /
        select_action / select_action_chunk, rtc with either method -- (fv_head_set_flow_solver).  flow_steps keeps meaning steps: a sample costs flow_steps x
        (1, 2, 2, 4) network evaluations, and at an equal number of evaluations a higher-order solver ends one to two orders closer to the exact flow
        (DESIGN.md section 7); action_error_per_dim(batch) is the action-space metric to choose a solver and a step count with.  policy.flow_solver may be
        changed at any time on a policy BUILT with a higher-order solver (the workspace holds their two rows); a policy built with "euler" raises ValueError.
        A property of the run: hip_extras.json records it only when it is not Euler.  ValueError with a regression head.

        flow_samples=S (flow head, 1 .. 16, default 1; FASTVLA_FLOW_SAMPLES) with flow_select="medoid" (the default with S > 1) | "coherent" | "first"
        (FASTVLA_FLOW_SELECT): predict / select_action / select_action_chunk draw S candidate chunks per observation in ONE sampler call
        (fv_head_flow_sample_multi; candidate s is the single sample at offset + (s << 56), so "first" serves the bits of a policy without samples) and
        return one of them, chosen on the device: the medoid (the candidate the others agree with), or the one that best continues the chunk planned last
        over the steps the two share, step k weighted flow_coherence_decay**k (default 0.5; FASTVLA_FLOW_COHERENCE_DECAY; the backward-coherence criterion of
        Bidirectional Decoding, Liu et al. 2024).  "coherent" keeps the chosen chunk: select_action scores a re-plan against it read `shift` = the actions
        served since steps ahead, the first plan after reset() takes the medoid, and predict -- a call on its own -- takes the medoid too; it works without
        rtc and with rtc_method="prefix" (every candidate then pins the same steps).  The candidates never average: between two modes the mean is a chunk the
        policy did not learn.  policy.last_candidates (B, S, K, A, normalised), last_choice (B) and last_sample_spread (B, K, A; the candidates' standard
        deviation, an uncertainty signal) stay on the device.  The queue, n_action_steps, temporal ensembling, the solver and flow_steps work on the chosen
        chunk; action_error_per_dim stays single-sample.  A property of the run: no checkpoint or hip_extras.json key.  ValueError, before any engine exists,
        for a regression head, S outside 1 .. 16, a select name with S = 1, "coherent" with chunk_size = 1, rtc_method="guidance" with S > 1.

        action_head="bins" (OpenVLA / RT-2 "discretised actions"; normalised action space): every action element is a classification over action_bins = Nb
        (2 .. 1024, default 256; FASTVLA_ACTION_BINS) uniform bins of action_bins_range = (lo, hi), or one pair per action dimension (default (-3, 3);
        FASTVLA_ACTION_BINS_RANGE="lo:hi"; fastvla_hip.engine.bins_ranges_from_stats turns dataset min / max / mean / std into per-dimension pairs).  The same
        12 tensors, action_head.weight Nb times taller: an ARCHITECTURE property, recorded in hip_extras.json, and a checkpoint of another head type does not
        load.  Training is the cross-entropy of the logits against the target's bin (targets clamped to the range), with the chunk mask, the loss weights and
        the all-elements denominator of every other loss; action_bins_sigma = s > 0 (FASTVLA_ACTION_BINS_SIGMA; HL-Gauss, Farebrother et al. 2024, 0.75 is their
        recommendation) smooths the one-hot target into a Gaussian of s bin widths integrated over the bins.  action_bins_decode "argmax" (default) | "mean"
        (FASTVLA_ACTION_BINS_DECODE): predict / select_action / select_action_chunk return the centre of the most likely bin, or the mean of the centres under
        the softmax; the queue, n_action_steps and temporal ensembling work on the decoded chunk.  compute_loss / forward(batch) / the train step return the
        decoded chunk (normalised) beside the loss, and last_loss_metrics / the step's "accuracy" the fraction of valid elements whose most likely bin is the
        target's.  action_bin_probs(batch) -> (B, K, A, Nb) on the device.  The twins are read for a bins head only.  ValueError, naming both settings and
        before any engine exists: bins with any flow_* / rtc* option or an action_loss other than "mse", an action_bins_* option with another head, Nb outside
        2 .. 1024, chunk_size * action_dim * Nb > 32768, lo >= hi, a range list that is neither one pair nor action_dim pairs, a negative sigma, an unknown
        decode; predict with autograd enabled on the head raises ValueError too (the decode is not differentiated)."""
        super().__init__()
        self.config = config or FastVLAConfig()
        self.options = resolve_policy_options(      # (every option is resolved and refused here, before any engine exists)
            chunk_size=chunk_size, n_action_steps=n_action_steps, action_loss=action_loss, action_loss_beta=action_loss_beta,
            temporal_ensemble_coeff=temporal_ensemble_coeff, action_dim_weights=action_dim_weights, action_step_weights=action_step_weights,
            action_head=action_head, flow_steps=flow_steps, flow_time_dim=flow_time_dim, flow_time_dist=flow_time_dist, flow_time_range=flow_time_range,
            flow_time_stratify=flow_time_stratify, flow_seed=flow_seed, rtc=rtc, rtc_schedule=rtc_schedule, rtc_max_guidance_weight=rtc_max_guidance_weight, rtc_execution_horizon=rtc_execution_horizon,
            flow_noise_draws=flow_noise_draws, flow_prefix_max_delay=flow_prefix_max_delay, flow_prefix_delay_dist=flow_prefix_delay_dist,
            flow_prefix_delay_rate=flow_prefix_delay_rate, rtc_method=rtc_method, rtc_prefix_steps=rtc_prefix_steps, flow_solver=flow_solver,
            flow_samples=flow_samples, flow_select=flow_select, flow_coherence_decay=flow_coherence_decay, action_bins=action_bins,
            action_bins_range=action_bins_range, action_bins_sigma=action_bins_sigma, action_bins_decode=action_bins_decode, action_dim=self.config.action_dim)
        o = self.options
        self.n_action_steps = o.chunk["n_action_steps"]
        self.temporal_ensemble_coeff: Optional[float] = o.chunk["temporal_ensemble_coeff"]
        self.action_head, self.flow_noise_draws, self.flow_prefix, self.rtc = o.action_head, o.noise_draws, o.prefix, o.rtc
        self.flow_samples, self.flow_select = o.samples, o.select
        self._ensembler = None      # fastvla_hip.TemporalEnsembler, created on the first select_action after reset()
        self._action_queue: deque = deque()
        self._rtc_served = 0      # actions served since the last chunk was planned: the shift of the next guided plan
        self.model = FastVLMWithExpert(self.config, o)
        self.processor = FastVLAProcessor(self.config, self.model.backbone)
        self._opt_state = None
        self._unfrozen = None   # training/unfrozen.py UnfrozenState once enable_backbone_training() ran

    def enable_backbone_training(self, bucket_min_numel: int = 1 << 22, tower: Optional[bool] = None, lora_rank: Optional[int] = None,
                                 lora_alpha: Optional[float] = None, lora_targets=None, lora_seed: int = 0, lora_direct: Optional[bool] = None,
                                 lora_dora: Optional[bool] = None, lora_rslora: Optional[bool] = None, lr_scales: Optional[Dict] = None, no_decay=None,
                                 layer_decay: Optional[float] = None, lora_plus_ratio: Optional[float] = None, freeze=None):
        """Extension of this build: fine-tune the Qwen2 decoder + mm_projector together with the action expert
        (image tokens spliced); tower=True (or FASTVLA_TRAIN_TOWER=1) trains the FastViT-HD tower too, in its inference form, otherwise it stays
        frozen.  Explicit on purpose: the reference's `freeze_backbone=False` trains nothing but the head either (model/fastvlm_adapter.py:501),
        so the config flag alone must not change what a step computes.

        lora_rank=r (1 .. 64; or FASTVLA_LORA_RANK, with FASTVLA_LORA_ALPHA / FASTVLA_LORA_TARGETS): LoRA mode -- the decoder's matrices stay frozen and the
        target matrices (default all seven: q, k, v, o, gate, up, down) run as W0 + (lora_alpha / r) B A (default alpha = r), action expert and mm_projector
        train in full; gradients, Adam's moments and the data-parallel exchange cover the trainable tensors only.  Not together with tower=True.

        lora_direct=True (with lora_rank; or FASTVLA_LORA_DIRECT=1): the DIRECT LoRA backward -- dA / dB straight from activations and output gradients
        (fv_train_lora_forward_backward); the full-size gradient buffer is never allocated.  A property of the run, not of the adapters: adapter and optimiser
        files written in one mode load in the other; a state that is already running keeps the mode it was started in (lora_direct=None), and asking it
        for the other mode explicitly raises RuntimeError.

        lora_rslora=True (or FASTVLA_LORA_RSLORA=1): rank-stabilised scaling, W0 + (lora_alpha / sqrt(r)) B A.  lora_dora=True (or FASTVLA_LORA_DORA=1):
        weight-decomposed LoRA (PEFT's use_dora) -- a trained magnitude per output row over the direction W0 + s B A, initialised to the row norms so the
        adapted model starts as the base model.  Both ARE properties of the adapters: they are recorded with {rank, alpha, targets} wherever those travel.
        DoRA runs on the projected backward only: lora_dora=True with lora_direct=True raises ValueError.

        Parameter groups of the optimiser step (fastvla_hip/optim.py; fv_adamw_clip_step_groups), each with an environment twin an explicit argument beats:
        lr_scales={"decoder": 0.1, "tower": 0.1} (FASTVLA_LR_SCALES="decoder=0.1,tower=0.1") -- learning-rate factors per section (head, projector, embedding,
        decoder, tower, adapters); no_decay=("vectors",) (FASTVLA_NO_DECAY) -- sections, or the class "vectors" (norm weights, biases, layer scales, DoRA
        magnitudes), without weight decay; layer_decay=d (FASTVLA_LAYER_DECAY) -- decoder layer l of L, and its adapters, x d^(L-1-l), the embedding x d^L;
        lora_plus_ratio=r (FASTVLA_LORA_PLUS_RATIO; needs LoRA, ValueError otherwise) -- lora_B at r times lora_A's rate; freeze=("embedding",)
        (FASTVLA_FREEZE) -- sections or "vectors" left untouched and out of the clip norm.  Factors multiply.  With none of them the step is the single-group
        one, bit for bit.  The step then also returns "group_grad_norms" (a device tensor, one norm per group) and "group_names" (their labels)."""
        from fastvla_hip import lora as _lora
        self._ema_refuse_in_scope("enable_backbone_training()")
        if tower is None:
            tower = os.environ.get("FASTVLA_TRAIN_TOWER", "0") == "1"
        if lora_rank is None and lora_alpha is None and lora_targets is None:
            if (lora_dora or lora_rslora) and (os.environ.get("FASTVLA_LORA_RANK") or "").strip() in ("", "0"):
                raise ValueError("lora_dora / lora_rslora need a rank (lora_rank or FASTVLA_LORA_RANK)")
            lcfg = _lora.config_from_env()       # the environment twins, in the style of FASTVLA_TRAIN_TOWER
            if lcfg is not None:                 # (an explicit argument beats its environment twin)
                for key, arg in (("dora", lora_dora), ("rslora", lora_rslora)):
                    if arg is not None:
                        lcfg.pop(key, None)
                        if arg:
                            lcfg[key] = True
            if lcfg is None and (lora_direct or (lora_direct is None and _lora.direct_from_env())):
                raise ValueError("lora_direct / FASTVLA_LORA_DIRECT need a rank (lora_rank or FASTVLA_LORA_RANK)")
            if lcfg is not None and tower:
                raise ValueError("FASTVLA_LORA_RANK and a trained tower (tower=True / FASTVLA_TRAIN_TOWER=1) cannot be combined: LoRA adapters go with a frozen vision tower")
        else:
            if lora_rank is None:
                raise ValueError("lora_alpha / lora_targets / lora_direct need lora_rank")
            var = _lora.variants_from_env()
            lcfg = _lora.check_config(lora_rank, lora_alpha, lora_targets, tower=bool(tower), dora=var.get("dora", False) if lora_dora is None else lora_dora,
                                      rslora=var.get("rslora", False) if lora_rslora is None else lora_rslora)
        if lcfg is not None and lcfg.get("dora") and (lora_direct or (lora_direct is None and self._unfrozen is None and _lora.direct_from_env())):
            raise ValueError("lora_dora and lora_direct cannot be combined: DoRA's magnitude gradient needs the full weight gradient (the projected backward)")
        if self._unfrozen is not None and bool(tower) and not self._unfrozen.train_tower:
            raise RuntimeError("backbone training is already running with the tower frozen: ask for tower=True on the first call")
        if self._unfrozen is not None and lcfg is not None and self._unfrozen.lora != lcfg:
            raise RuntimeError(f"backbone training is already running with lora={self._unfrozen.lora}: ask for LoRA on the first call")
        if self._unfrozen is not None and lcfg is not None and lora_direct is not None and bool(lora_direct) != self._unfrozen.lora_direct:
            raise RuntimeError(f"backbone training is already running with lora_direct={self._unfrozen.lora_direct}: ask for the backward mode on the first call")
        from fastvla_hip import optim as _optim
        given = {k: v for k, v in (("lr_scales", lr_scales), ("no_decay", no_decay), ("layer_decay", layer_decay), ("lora_plus_ratio", lora_plus_ratio),
                                   ("freeze", freeze)) if v is not None}
        if self._unfrozen is not None:
            if given and _optim.normalize_options(**given) != self._unfrozen.optim:
                raise RuntimeError(f"backbone training is already running with the optimiser options {self._unfrozen.optim}: ask for parameter groups on the first call")
        else:
            opts = {**_optim.options_from_env(), **_optim.normalize_options(**given)}      # (an explicit argument beats its environment twin)
            for k, v in given.items():       # ... also when it switches the twin OFF (an empty tuple / dict)
                if k not in _optim.normalize_options(**{k: v}):
                    opts.pop(k, None)
            if "lora_plus_ratio" in opts and lcfg is None:
                raise ValueError("lora_plus_ratio / FASTVLA_LORA_PLUS_RATIO need LoRA adapters (lora_rank or FASTVLA_LORA_RANK)")
            from ..training.unfrozen import UnfrozenState
            direct = lcfg is not None and (_lora.direct_from_env() if lora_direct is None else bool(lora_direct))
            self._unfrozen = UnfrozenState(self, bucket_min_numel=bucket_min_numel, train_tower=bool(tower), lora=lcfg, lora_seed=lora_seed, lora_direct=direct,
                                           optim=opts)
            self._ema_attach()      # (EMA switched on before this call: the average restarts as a copy of the new trainable buffer)
        return self._unfrozen

    def enable_image_augmentation(self, crop_area=None, crop_ratio=None, brightness=None, contrast=None, saturation=None, seed: Optional[int] = None,
                                  value_max: Optional[float] = None) -> Dict:
        """Extension of this build: random crop + brightness / contrast / saturation jitter of TRAINING batches, drawn and applied on the device inside the
        letterbox call (FastVLMBackbone.enable_image_augmentation has the details; fastvla_hip/augment.py the semantics).  Ranges are (lo, hi) or a number;
        with none given FASTVLA_IMAGE_AUG decides, else the preset `default` (crop_area 0.9, colour factors 0.8 .. 1.2); seed: FASTVLA_IMAGE_AUG_SEED, else 0.
        Only prepare_batch / the unfrozen prepare of a policy in train() mode augment: select_action, compute_loss, Trainer.evaluate and already
        prepared pixels never do.  The image tokens reach the action in splice mode only (backbone training forces it)."""
        return self.model.backbone.enable_image_augmentation(crop_area=crop_area, crop_ratio=crop_ratio, brightness=brightness, contrast=contrast,
                                                             saturation=saturation, seed=seed, value_max=value_max)

    def disable_image_augmentation(self) -> None:
        self.model.backbone.disable_image_augmentation()

    def merge_lora(self) -> None:
        """LoRA mode: fold the adapters into the fp32 master (W0 += s B A, lora_B = 0).  The model computes what it computed before; the backbone export
        (save_policy_checkpoint(include_backbone=True), FASTVLA_SAVE_BACKBONE) then writes a plain checkpoint under the reference's keys."""
        if self._unfrozen is None or self._unfrozen.lora is None:
            raise RuntimeError("merge_lora(): this policy has no LoRA adapters (enable_backbone_training(lora_rank=...))")
        self._ema_refuse_in_scope("merge_lora()")
        self._unfrozen.merge_lora()

    def forward(self, images: torch.Tensor, states: torch.Tensor, tasks: List[str] | str,
                device: torch.device | None = None) -> torch.Tensor:
        if device is None:
            device = images.device
        images = self.processor.prepare_images(images, device)
        states = self.processor.prepare_states(states, device)
        tasks = self.processor.prepare_tasks(tasks, batch_size=images.shape[0])
        return self.model(images, states, tasks, device=device)

    def compute_loss(self, batch: Dict[str, torch.Tensor | List[str]]) -> Dict[str, torch.Tensor]:
        """reference fastvla/modeling_fastvla.py:52-57: {"loss": mse (differentiable w.r.t. the head), "mse": detached}.
        Head forward, MSE and the head gradients come from one pass through the library (no torch operator in between)."""
        images, states, tasks = batch["images"], batch["states"], batch["tasks"]
        device = images.device
        images = self.processor.prepare_images(images, device)
        states = self.processor.prepare_states(states, device)
        tasks = self.processor.prepare_tasks(tasks, batch_size=images.shape[0])
        loss, _pred = self.model.forward_loss(images, states, tasks, batch["actions"], device=device, pad=batch.get("action_is_pad"))
        met = self.model.last_loss_metrics      # None on the plain MSE path: "mse" is then the loss itself, as ever
        out = {"loss": loss, "mse": loss.detach() if met is None else met[0]}
        if self.model.bins is not None:      # a binned head: the loss is a cross-entropy, "mse" the decoded chunk's masked squared error
            out["accuracy"] = met[2]
        return out

    def set_action_loss(self, kind: str, beta: float = 1.0) -> None:
        """the loss of every later compute_loss / train step: "mse" | "l1" | "smooth_l1" (beta)"""
        self.model.set_action_loss(kind, beta)

    def set_action_loss_weights(self, dim_weights=None, step_weights=None) -> None:
        """weights of the loss of every later compute_loss / train step, on every training route: dim_weights (A values), step_weights (K values); both None
        switches weighting off"""
        self.model.set_action_loss_weights(dim_weights, step_weights)

    @torch.no_grad()
    def action_error_per_dim(self, batch: Dict[str, torch.Tensor | List[str]]) -> torch.Tensor:
        """-> (A,): mean |prediction - target| per action dimension over the batch's non-padded steps (normalised space, unweighted): what the per-dimension
        weights are tuned against.  Runs on demand, outside the train step.  A flow head samples one chunk per row with policy.flow_solver and
        policy.flow_steps from noise at a fixed offset of the flow seed: repeatable, and the sampling counter does not advance."""
        images, states, tasks = batch["images"], batch["states"], batch["tasks"]
        device = images.device
        images = self.processor.prepare_images(images, device)
        states = self.processor.prepare_states(states, device)
        tasks = self.processor.prepare_tasks(tasks, batch_size=images.shape[0])
        targets, pad = self.model.chunk_targets(batch["actions"], batch.get("action_is_pad"))
        pooled = self.model.features(images, tasks, device=device)
        return self.model.action_error_per_dim(pooled, states, targets, pad)

    @property
    def last_loss_metrics(self) -> Optional[torch.Tensor]:
        """what the last compute_loss / forward(batch) left beside its loss: (2,) [masked MSE, valid fraction] from the chunked kernel, (3,) with the bin
        accuracy behind them for a binned head, None on the plain MSE path"""
        return self.model.last_loss_metrics

    @torch.no_grad()
    def action_bin_probs(self, batch: Dict[str, torch.Tensor | List[str]]) -> torch.Tensor:
        """-> (B, K, A, action_bins) on the device: a binned head's distribution over the bins of every action element (its entropy is an uncertainty signal)"""
        images, states, tasks = batch["images"], batch["states"], batch["tasks"]
        device = images.device
        images = self.processor.prepare_images(images, device)
        states = self.processor.prepare_states(states, device)
        tasks = self.processor.prepare_tasks(tasks, batch_size=images.shape[0])
        return self.model.action_bin_probs(self.model.features(images, tasks, device=device), states)

    @torch.no_grad()
    def flow_loss_per_time(self, batch: Dict[str, torch.Tensor | List[str]], buckets: int = 10):
        """-> (mse, count), each (buckets,) on the device: the velocity error of the flow head by time bucket over the batch's non-padded steps (normalised
        space, unweighted) -- the metric a time distribution (flow_time_dist, flow_time_range) is judged with.  One backbone forward; head row r is noised at
        the explicit time ((r mod buckets) + 0.5) / buckets from noise at a fixed offset of the flow seed: repeatable, no dropout, no counter advances."""
        images, states, tasks = batch["images"], batch["states"], batch["tasks"]
        device = images.device
        images = self.processor.prepare_images(images, device)
        states = self.processor.prepare_states(states, device)
        tasks = self.processor.prepare_tasks(tasks, batch_size=images.shape[0])
        targets, pad = self.model.chunk_targets(batch["actions"], batch.get("action_is_pad"))
        pooled = self.model.features(images, tasks, device=device)
        return self.model.flow_loss_per_time(pooled, states, targets, pad, buckets)

    @property
    def chunk_size(self) -> int:
        return self.model.chunk_size

    @torch.inference_mode()
    def select_action_chunk(self, image: torch.Tensor, state: torch.Tensor, task: str, device: torch.device, prev_chunk: Optional[torch.Tensor] = None,
                            inference_delay: Optional[int] = None, num_samples: Optional[int] = None) -> torch.Tensor:
        """-> (K, A): the whole chunk the head predicts for one observation (K = chunk_size; (1, A) without chunks).
        rtc=True: prev_chunk (K', A), K' <= K, in NORMALISED space -- the not-yet-executed rows of the previous chunk, policy.last_chunk_normalised[executed:] --
        guides the sample (row k of the new chunk towards row k of prev_chunk), with the first inference_delay steps as a hard prefix: the explicit form for
        callers that plan while the previous chunk is still being executed.  Without prev_chunk the sample is guided by the chunk the policy planned last
        (none after reset(): unguided), read from its start.  inference_delay None: 0 under rtc_method="guidance"; under rtc_method="prefix" the policy's
        rtc_prefix_steps, as in select_action (rows without a previous chunk pin nothing whatever the delay).
        num_samples (flow_samples > 1; 1 .. flow_samples): the candidates of THIS call; the chosen chunk is returned.  flow_select="coherent" scores them
        against the chunk planned last, read from its start (none after reset(): the medoid), and keeps the chosen one."""
        if num_samples is not None:
            from fastvla_hip.select import check_flow_samples
            if check_flow_samples(num_samples) > self.flow_samples:
                raise ValueError(f"num_samples={num_samples} exceeds the flow_samples={self.flow_samples} the policy was constructed with (the sampler's rows are sized for it)")
            self.model.flow_samples_now = int(num_samples)
            try:
                return self.select_action_chunk(image, state, task, device, prev_chunk=prev_chunk, inference_delay=inference_delay)
            finally:
                self.model.flow_samples_now = self.flow_samples
        self.eval()
        if self.rtc is None and self.flow_select == "coherent":
            if prev_chunk is not None or inference_delay not in (None, 0):
                raise ValueError(f"prev_chunk / inference_delay need rtc=True. Got inference_delay={inference_delay}, rtc={self.rtc is not None}.")
            return self._coherent_plan(image, state, task, device, shift=0)
        if self.rtc is None:
            if prev_chunk is not None or inference_delay not in (None, 0):
                raise ValueError(f"prev_chunk / inference_delay need rtc=True. Got inference_delay={inference_delay}, rtc={self.rtc is not None}.")
            tasks = self.processor.prepare_tasks(task, batch_size=1)
            action = self.forward(image.unsqueeze(0).to(device), state.unsqueeze(0).to(device), tasks, device=device)
            return action.reshape(self.model.chunk_size, self.config.action_dim)
        K, A = self.model.chunk_size, self.config.action_dim
        prev, shift = None, 0
        if prev_chunk is not None:
            rows = torch.as_tensor(prev_chunk, dtype=torch.float32).reshape(-1, A)
            if not 1 <= rows.shape[0] <= K:
                raise ValueError(f"prev_chunk must hold 1 .. chunk_size = {K} rows of {A} values, got {tuple(rows.shape)}")
            shift = K - rows.shape[0]      # the rows sit at the END of a full chunk, which the sampler reads `shift` steps ahead
            prev = torch.zeros(1, K, A, dtype=torch.float32, device=device)
            prev[0, shift:] = rows.to(device)
        return self._rtc_plan(image, state, task, device, shift=shift, inference_delay=inference_delay, prev=prev)

    def _rtc_plan(self, image, state, task, device, *, shift: int, inference_delay: Optional[int] = None, prev=None) -> torch.Tensor:
        images = self.processor.prepare_images(image.unsqueeze(0).to(device), device)
        states = self.processor.prepare_states(state.unsqueeze(0).to(device), device)
        tasks = self.processor.prepare_tasks(task, batch_size=1)
        pooled = self.model.features(images, tasks, device=device)
        chunk = self.model.rtc_sample(pooled, states, shift=shift, inference_delay=inference_delay, prev=prev)
        self._rtc_served = 0
        return chunk.reshape(self.model.chunk_size, self.config.action_dim)

    def _coherent_plan(self, image, state, task, device, *, shift: int) -> torch.Tensor:
        """flow_select="coherent" without rtc: flow_samples candidates, the one that best continues the chunk planned last (read `shift` steps ahead) chosen"""
        images = self.processor.prepare_images(image.unsqueeze(0).to(device), device)
        states = self.processor.prepare_states(state.unsqueeze(0).to(device), device)
        tasks = self.processor.prepare_tasks(task, batch_size=1)
        pooled = self.model.features(images, tasks, device=device)
        chunk = self.model.sample_multi(pooled, states, shift=shift)
        self._rtc_served = 0
        return chunk.reshape(self.model.chunk_size, self.config.action_dim)

    @property
    def last_chunk_normalised(self) -> Optional[torch.Tensor]:
        """rtc=True: (K, A) copy of the last planned chunk in normalised space (before the folded dataset statistics), None before the first plan"""
        last = self.model.last_chunk_normalised
        return None if last is None else last[0]

    @torch.inference_mode()
    def select_action(self, image: torch.Tensor, state: torch.Tensor, task: str, device: torch.device) -> torch.Tensor:
        """One action (A,) per environment step.  With n_action_steps = n > 1 the backbone runs on every n-th call: the first n rows of the predicted chunk
        are queued and served in order; reset() empties the queue.  With temporal_ensemble_coeff set the backbone runs on every call and the action is the
        ensembler's weighted mean over the chunks predicted since reset() (no host synchronisation: the mean lives on the device)."""
        if self.temporal_ensemble_coeff is not None:
            chunk = self.select_action_chunk(image, state, task, device)
            return self._temporal_ensembler(1).step(chunk.reshape(1, self.model.chunk_size, self.config.action_dim))[0]
        if self.rtc is not None:
            if not self._action_queue:   # the re-plan is guided by the last chunk, read from the first step that has not been served yet
                self.eval()
                self._action_queue.extend(self._rtc_plan(image, state, task, device, shift=self._rtc_served)[: self.n_action_steps].unbind(0))
            self._rtc_served += 1
            return self._action_queue.popleft()
        if self.flow_select == "coherent":      # (without rtc: the re-plan is the candidate that best continues the last chunk from the first step not served yet)
            if not self._action_queue:
                self.eval()
                self._action_queue.extend(self._coherent_plan(image, state, task, device, shift=min(self._rtc_served, self.model.chunk_size))[: self.n_action_steps].unbind(0))
            self._rtc_served += 1
            return self._action_queue.popleft()
        if not self._action_queue:       # (n_action_steps = 1: a prediction on every call, row 0 served)
            self._action_queue.extend(self.select_action_chunk(image, state, task, device)[: self.n_action_steps].unbind(0))
        return self._action_queue.popleft()

    def _temporal_ensembler(self, n_env: int):
        from fastvla_hip.ensemble import TemporalEnsembler
        eng, ens = self.model._engine(), self._ensembler
        if ens is None or ens._engine is not eng or not ens._h:      # (the first call after reset(), or the engine was rebuilt underneath)
            ens = self._ensembler = TemporalEnsembler(eng, n_env, self.model.chunk_size, self.config.action_dim, self.temporal_ensemble_coeff)
        return ens

    def reset(self) -> None:
        self._action_queue.clear()
        self._rtc_served = 0
        self.model.rtc_reset()      # (rtc: the next plan is unguided)
        if self._ensembler is not None:
            self._ensembler.close()
            self._ensembler = None

    # ------------------------------------------------------------------ native train step
    def prepare_batch(self, batch: Dict[str, torch.Tensor | List[str]]) -> Dict[str, torch.Tensor]:
        """Everything of a train step that does NOT depend on the trainable parameters: image prep, tokenisation and the
        frozen backbone forward (reference model/fastvlm_adapter.py:501: no_grad, frozen) -> pooled features.  Enqueued on
        the current stream; a pipelined loop calls it for batch k+1 while batch k's gradient all-reduce is in flight."""
        m = self.model
        dev = m.backbone.engine().device
        images = self.processor.prepare_images(batch["images"], dev, augment=self.training)     # (image augmentation, when on: training batches only)
        states = self.processor.prepare_states(batch["states"], dev).float()
        tasks = self.processor.prepare_tasks(batch["tasks"], batch_size=images.shape[0])
        targets, pad = m.chunk_targets(batch["actions"].to(dev, torch.float32), batch.get("action_is_pad"))
        with torch.no_grad():
            pooled = m.features(images, tasks, device=dev)
        prep = {"pooled": pooled, "states": states, "targets": targets.contiguous()}
        if pad is not None:      # (B, K) bool: it travels with the prepared batch and reaches the handle only around this batch's own loss call
            prep["pad"] = pad.to(dev)
        return prep

    def _optimizer_state(self, flat: torch.Tensor) -> Dict:
        st = self._opt_state
        if st is None or st.get("flat") is not flat:
            from ..training.dp import GradExchange
            dev = flat.device
            keep = st or {}
            st = dict(m=torch.zeros_like(flat), v=torch.zeros_like(flat), g=torch.zeros_like(flat), acc=None, step=0, micro=0,
                      flat=flat, exchange=GradExchange(dev), norm=torch.zeros(1, device=dev), loss=torch.zeros(1, device=dev))
            if "resume" in keep:  # load_optimizer_state() ran before the flat buffer existed
                r = keep["resume"]
                st["m"].copy_(r["m"].to(dev))
                st["v"].copy_(r["v"].to(dev))
                st["step"] = int(r["step"])
            self._opt_state = st
        return st

    def load_optimizer_state(self, m: torch.Tensor, v: torch.Tensor, step: int, flat: Optional[torch.Tensor] = None,
                             train_tower: Optional[bool] = None, lora: Optional[Dict] = None, optim: Optional[Dict] = None) -> None:
        """Restore AdamW moments and the bias-correction step (Trainer._load_checkpoint; reference trainer.py:257-262
        restores them through accelerator.load_state).  train_tower: what optimizer.pt recorded about the run being resumed (None: a round-5 file, which
        did not record it -- FASTVLA_TRAIN_TOWER decides then, as before).  optim: the parameter-group options optimizer.pt recorded ({} = none): a run
        that steps with other options raises ValueError naming both."""
        head_numel = sum(p.numel() for p in self.model.head_parameters())
        if self._unfrozen is None and (train_tower is not None or lora is not None or m.numel() > 2 * head_numel):
            # moments of a whole-backbone run (training/unfrozen.py writes one flat m / v over every trainable tensor): the run resumes unfrozen,
            # training what the checkpointed run trained (lora: optimizer.pt's record of a LoRA run -- its m / v / flat cover the trainable buffer)
            # (optim: the run's parameter-group options as optimizer.pt recorded them -- they come back with the run unless this one asks for others, which raises below)
            from fastvla_hip import optim as _optim
            okw = _optim.explicit_kwargs(optim) if optim and not _optim.options_from_env() else {}
            if lora is not None:
                self.enable_backbone_training(lora_rank=lora["rank"], lora_alpha=lora["alpha"], lora_targets=lora["targets"],
                                              lora_dora=bool(lora.get("dora")), lora_rslora=bool(lora.get("rslora")), **okw)
            else:
                self.enable_backbone_training(tower=train_tower, **okw)
        if self._unfrozen is not None:
            u = self._unfrozen
            if optim is not None:      # (None: a caller that does not know what the checkpointed run used)
                from ..utils.checkpoint import check_resume_optim
                check_resume_optim(optim, u.optim)
            if m.numel() != u.m.numel():
                raise ValueError(f"optimizer state has {m.numel()} elements, the trainable tensors of this run {u.m.numel()} (tower trained in one run and frozen in the other?)")
            u.m.copy_(m.to(u.m.device))
            u.v.copy_(v.to(u.v.device))
            u.step_count = int(step)
            self._opt_state["step"] = int(step)
            if flat is not None:      # the fp32 master of the run being resumed (Trainer._save_checkpoint): parameters continue bit for bit
                if flat.numel() != u.trainable.numel():       # (LoRA mode: the trainable buffer -- head, projector, adapters)
                    raise ValueError(f"checkpointed master has {flat.numel()} elements, this run's {u.trainable.numel()}")
                u.trainable.copy_(flat.to(u.trainable.device))
                u.commit()
            return
        flat = self.model._flat
        if flat is None:
            self._opt_state = {"resume": {"m": m, "v": v, "step": int(step)}}
            return
        st = self._optimizer_state(flat)
        st["m"].copy_(m.to(flat.device))
        st["v"].copy_(v.to(flat.device))
        st["step"] = int(step)

    def fused_train_step(self, batch: Optional[Dict] = None, *, lr: float, betas=(0.9, 0.95), eps: float = 1e-8,
                         weight_decay: float = 1e-4, max_grad_norm: Optional[float] = 1.0, process_group=None,
                         prepared: Optional[Dict] = None, next_batch: Optional[Dict] = None,
                         grad_accum_steps: int = 1, force_sync: bool = False) -> Dict[str, torch.Tensor]:
        """One pass of the step body of reference training/trainer.py:171-182 (loss -> backward -> [accumulate] -> clip ->
        AdamW), entirely on the HIP path.

        * grad_accum_steps = k: the flat gradient is summed over k calls (fv_grad_accumulate); the exchange, the clip and
          the optimiser run on every k-th call -- or when `force_sync` says the loader is exhausted -- with the 1/k of
          accelerate's `accumulate` folded into the optimiser's grad_scale (trainer.py:96,171).
        * under torch.distributed the accumulated gradient is summed across ranks with ONE all-reduce on a side stream
          (1/world folded into grad_scale as well).  When `next_batch` is given, ITS frozen backbone forward is enqueued
          between the start of the all-reduce and the optimiser kernel, so the collective runs underneath it; the
          prepared batch comes back under "next" and is passed as `prepared=` to the following call.
        * with EMA on (enable_ema() or FASTVLA_EMA_DECAY; fastvla/ema_state.py) the optimiser call of a synced micro-batch also moves the average of the
          trainable buffer (fv_adamw_clip_step_ema) and the result gains "ema_weight", the weight 1 - d_t of the last update.
        * with the step guard on (enable_step_guard() or FASTVLA_STEP_GUARD=1; fastvla/guard_state.py) the optimiser call is fv_adamw_clip_step_guarded: a
          step whose gradient is non-finite (backbone training: or whose fp16 operands saturated) is skipped on the device, and the result gains
          "step_skipped" (0 / 1: the last guarded step's decision) and "loss_scale" (the scale the next backward runs with), both device tensors.  `step`,
          Adam's bias-correction index, advances on a skipped step too.
        """
        self._ema_from_env()
        self._step_guard_from_env()
        self._ema_refuse_in_scope("a training step")
        if self._unfrozen is None and not self.config.freeze_backbone and os.environ.get("FASTVLA_TRAIN_BACKBONE", "0") == "1":
            self.enable_backbone_training()
        if self._unfrozen is not None:
            out = self._unfrozen.step(batch, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                      process_group=process_group, prepared=prepared, grad_accum_steps=grad_accum_steps, force_sync=force_sync)
            if self.training:
                self.model.backbone.note_train_step()     # (the augmentation's batch counter: what a checkpoint records)
            if self._ema is not None:
                out["ema_weight"] = self._ema["weight"]
            if next_batch is not None:
                # Trainer's one batch of look-ahead (training/trainer.py _train_one_epoch): an unfrozen forward depends on the update, so only the
                # parameter-INDEPENDENT half of the next batch is prepared here, AFTER the commit (image prep, tokenisation, the tower while it is frozen)
                out["next"] = self._unfrozen.prepare(next_batch)
            return out
        m = self.model
        prep = prepared if prepared is not None else self.prepare_batch(batch)
        if self.training:
            m.backbone.note_train_step()     # (the augmentation's batch counter: what a checkpoint records)
        dev = prep["pooled"].device
        eng, flat = m._engine(), m.materialize(dev)
        st = self._optimizer_state(flat)
        k = max(1, int(grad_accum_steps))
        st["micro"] += 1
        sync = force_sync or st["micro"] % k == 0
        p = float(self.config.dropout) if self.training else 0.0
        m._drop_calls += 1
        targets, saved = prep["targets"], None
        if m.flow is not None:      # flow head: noise the targets first (x_t, phi(t) into `saved`); the loss below then compares velocities
            saved = eng.head_saved(prep["pooled"].shape[0])
            seed, offset = m.flow_train_draw(st["step"], st["micro"]) if self.training else m.flow_eval_draw()
            targets = eng.head_flow_prepare(targets, saved, seed=seed, offset=offset)
        actions, saved = eng.head_forward(flat, prep["pooled"], prep["states"], training=p > 0.0, dropout_p=p,
                                          seed=m._drop_seed, offset=m._drop_calls, normalized_actions=True, saved=saved)
        if k > 1 and st["acc"] is None:
            st["acc"] = torch.zeros_like(flat)
        first = st["micro"] == 1  # first micro-batch of an accumulation window: the backward writes the window's buffer
        target_buf = st["g"] if k == 1 else (st["acc"] if first else st["g"])
        pad = prep.get("pad")
        loss, grads = eng.head_backward(flat, actions, targets, saved, dropout_p=p, flat_grads=target_buf, pad=pad)
        guard = self._step_guard_attach(eng, None)      # None with the guard off: every call below is then the one it was (head-only: fp32, delta stays 1)
        if guard is not None:
            guard.observe()
        if k > 1 and not first:
            eng.grad_accumulate(st["acc"], grads)
        total = st["g"] if k == 1 else st["acc"]
        actions = actions[:prep["pooled"].shape[0]]      # (flow_noise_draws > 1: every draw's rows, draw-major; the step hands out draw 0's velocity)
        met = eng.head_loss_metrics() if eng.loss_is_chunked(pad) else None
        out = {"loss": loss[0], "mse": met[0] if met is not None else loss[0].detach(), "actions": m._shape_actions(actions), "synced": sync, "next": None}
        if m.bins is not None:
            out["accuracy"] = met[2]
        scale = 1.0
        if sync:
            st["exchange"].group = process_group
            scale = st["exchange"].start(total) / k       # all-reduce launched on the side stream
        if next_batch is not None:
            out["next"] = self.prepare_batch(next_batch)  # frozen forward of batch k+1, underneath the collective
        if sync:
            st["exchange"].finish(dev)
            st["step"] += 1
            st["micro"] = 0
            gkw = {}
            if guard is not None:
                from fastvla_hip.guard import all_reduce_flag
                all_reduce_flag(guard.flag(), process_group)      # one rank's flag skips the step on every rank (a NaN / inf survives the gradient sum by itself)
                gkw["guard"] = guard
            eng.adamw_step(flat, total, st["m"], st["v"], st["step"], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                           max_grad_norm=max_grad_norm or 0.0, grad_scale=scale, grad_norm_out=st["norm"], **self._ema_step_args(st["step"]), **gkw)
        if guard is not None:
            rep = guard.report()
            out["step_skipped"], out["loss_scale"] = rep[0], rep[1]
        out["grad_norm"] = st["norm"][0]
        if self._ema is not None:
            out["ema_weight"] = self._ema["weight"]
        return out
