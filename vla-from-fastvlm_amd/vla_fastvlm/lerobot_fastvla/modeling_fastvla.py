"""LeRobot policy wrapper around FastVLMWithExpert (reference:
src/vla_fastvlm/lerobot_fastvla/modeling_fastvla.py:19-133): first VISUAL key, last timestep, task -> list[str] (+"\\n"),
forward(batch) -> (loss, {"loss","mse"}), predict_action_chunk -> [B,chunk_size,A], select_action with the action deque.

config.chunk_size = K > 1 (an extension of this build: the reference accepts the field and predicts one step) widens the head to K * A: the dataset's
(B, K, A) targets and its `action_is_pad` (B, K) train all K steps, padded ones excluded, and n_action_steps <= K of them are served per backbone run.
The loss kind ("mse" | "l1" | "smooth_l1") comes from set_action_loss() or FASTVLA_ACTION_LOSS / FASTVLA_ACTION_LOSS_BETA.

Temporal ensembling and loss weights (the registered config schema is pinned and gets no field): FastVLAPolicy(config, temporal_ensemble_coeff=c,
action_dim_weights=..., action_step_weights=...) or their FASTVLA_* twins.  With a coefficient select_action(batch) runs the backbone on every call and
ensembles all B environments of the batch on the device in one launch.

Real-time chunking of a flow head (no config field either): FastVLAPolicy(config, action_head="flow", rtc=True, rtc_schedule=, rtc_max_guidance_weight=,
rtc_execution_horizon=) or the FASTVLA_RTC* twins.  select_action(batch) then samples every re-plan guided by the rest of the previous chunk, for all B
environments in one call; predict_action_chunk(batch, inference_delay=, prev_chunk_left_over=, execution_horizon=) is LeRobot's keyword set.

Action-prefix conditioning (no config field): FastVLAPolicy(config, action_head="flow", flow_prefix_max_delay=D, flow_prefix_delay_dist=,
flow_prefix_delay_rate=) or the FASTVLA_FLOW_PREFIX_* twins train the head with a clean prefix of d <= D steps; rtc=True, rtc_method="prefix"
(FASTVLA_RTC_METHOD) then pins the first steps of every re-plan to the previous chunk with the plain sampler's three launches per step.

Higher-order integrators (no config field): FastVLAPolicy(config, action_head="flow", flow_solver="midpoint" | "heun" | "rk4") or FASTVLA_FLOW_SOLVER: every
sampling route -- predict_action_chunk, select_action, rtc with either method -- integrates with it, flow_steps being steps of the chosen solver;
policy.flow_solver switches among all four on a policy built with a higher-order one.

Several samples per observation (no config field): FastVLAPolicy(config, action_head="flow", flow_samples=S, flow_select="medoid" | "coherent" | "first",
flow_coherence_decay=) or the FASTVLA_FLOW_SAMPLES / FASTVLA_FLOW_SELECT / FASTVLA_FLOW_COHERENCE_DECAY twins: predict_action_chunk(batch, num_samples=) and
select_action draw S candidates per environment in one sampler call and return the one chosen on the device; last_candidates, last_choice and
last_sample_spread stay on the device.

Binned actions (no config field): FastVLAPolicy(config, action_head="bins", action_bins=, action_bins_range=, action_bins_sigma=, action_bins_decode=) or the
FASTVLA_ACTION_BINS* twins: forward(batch) trains the cross-entropy over the bins and reports {"loss", "mse", "accuracy"}, predict_action_chunk and
select_action return decoded chunks, action_bin_probs(batch) the (B, K, A, bins) distributions.  A torch optimiser sees the taller action_head through
forward(batch)'s gradients like any other head tensor."""
from __future__ import annotations

from collections import deque
from typing import Any

import torch
from torch import Tensor

from ..fastvla.configuration_fastvla import FastVLAConfig as CoreFastVLAConfig
from ..fastvla.fastvlm_with_expert import FastVLMWithExpert
from ..fastvla.flow_surface import FlowSurfaceMixin
from ..fastvla.options import POLICY_KEYWORDS, resolve_policy_options
from ._lerobot_compat import ACTION, FeatureType, PreTrainedPolicy
from .configuration_fastvla import FastVLAConfig

_CORE_FIELDS = ("vlm_model_name", "bootstrap_model_name", "state_dim", "action_dim", "hidden_dim", "fusion_dim", "dropout",
                "freeze_backbone", "tokenizer_max_length", "tokenizer_padding_side", "pad_to_max_length",
                "resize_with_padding", "image_size", "pad_value", "add_trailing_newline")


class FastVLAPolicy(PreTrainedPolicy, FlowSurfaceMixin):
    config_class = FastVLAConfig
    name = "fastvla"

    def __init__(self, config: FastVLAConfig, **kwargs: Any):
        super().__init__(config)
        config.validate_features()
        self.config = config
        self._state_key, self._image_keys = self._resolve_input_keys()
        self._infer_io_dims_from_features()
        # no option below has a field in the registered config (its schema is pinned): they come as keywords or from their FASTVLA_* twins, and the core
        # policy's docstring has their semantics.  Unknown keywords are ignored; the loss kind comes from its twins (or set_action_loss) only
        given = {k: v for k, v in kwargs.items() if k in POLICY_KEYWORDS}
        self.options = o = resolve_policy_options(**{**given, "chunk_size": config.chunk_size, "n_action_steps": config.n_action_steps, "action_loss": None,
                                                     "action_loss_beta": None, "action_dim": config.action_dim})
        self.temporal_ensemble_coeff = o.chunk["temporal_ensemble_coeff"]
        self.action_head, self.flow_noise_draws, self.flow_prefix, self.rtc = o.action_head, o.noise_draws, o.prefix, o.rtc
        self.flow_samples, self.flow_select = o.samples, o.select
        self._ensembler = None      # fastvla_hip.TemporalEnsembler over the B environments of select_action's batch, created on the first call after reset()
        self.model = FastVLMWithExpert(CoreFastVLAConfig(**{k: getattr(config, k) for k in _CORE_FIELDS}), o)
        self.reset()

    def set_action_loss(self, kind: str, beta: float = 1.0) -> None:
        """the loss forward(batch) evaluates from now on: "mse" | "l1" | "smooth_l1" (beta)"""
        self.model.set_action_loss(kind, beta)

    def set_action_loss_weights(self, dim_weights=None, step_weights=None) -> None:
        """weights of the loss forward(batch) evaluates from now on: dim_weights (A values), step_weights (K values); both None switches weighting off"""
        self.model.set_action_loss_weights(dim_weights, step_weights)

    @torch.no_grad()
    def action_error_per_dim(self, batch: dict[str, Tensor]) -> Tensor:
        """-> (A,): mean |prediction - target| per action dimension over the batch's non-padded steps (normalised space, unweighted).  A flow head samples
        one chunk per row with flow_solver and flow_steps from noise at a fixed offset of the flow seed: repeatable, the sampling counter does not advance"""
        images, states, tasks = self._prepare_inputs(batch)
        pad = batch.get("action_is_pad") if self.model.chunk_size > 1 else None
        targets, pad = self.model.chunk_targets(batch[ACTION], pad)
        pooled = self.model.features(images, tasks, device=images.device)
        return self.model.action_error_per_dim(pooled, states, targets, pad)

    @torch.no_grad()
    def action_bin_probs(self, batch: dict[str, Tensor]) -> Tensor:
        """-> (B, K, A, action_bins) on the device: a binned head's distribution over the bins of every action element"""
        images, states, tasks = self._prepare_inputs(batch)
        return self.model.action_bin_probs(self.model.features(images, tasks, device=images.device), states)

    def flow_loss_per_time(self, batch: dict[str, Tensor], buckets: int = 10):
        """-> (mse, count), each (buckets,) on the device: the flow head's velocity error by time bucket over the batch's non-padded steps (normalised space,
        unweighted).  Head row r is noised at the explicit time ((r mod buckets) + 0.5) / buckets from noise at a fixed offset of the flow seed: repeatable, no
        dropout, no counter advances"""
        images, states, tasks = self._prepare_inputs(batch)
        pad = batch.get("action_is_pad") if self.model.chunk_size > 1 else None
        targets, pad = self.model.chunk_targets(batch[ACTION], pad)
        pooled = self.model.features(images, tasks, device=images.device)
        return self.model.flow_loss_per_time(pooled, states, targets, pad, buckets)

    def _resolve_input_keys(self) -> tuple[str, list[str]]:
        feats = self.config.input_features
        if not feats:
            raise ValueError("FastVLA requires input_features to be set.")
        states = [k for k, ft in feats.items() if ft.type is FeatureType.STATE]
        images = [k for k, ft in feats.items() if ft.type is FeatureType.VISUAL]
        if not states:
            raise ValueError("No state feature found in input_features.")
        if not images:
            raise ValueError("No visual feature found in input_features.")
        return states[0], images

    def _infer_io_dims_from_features(self) -> None:
        feats = self.config.input_features
        if feats and self._state_key in feats:
            self.config.state_dim = feats[self._state_key].shape[0]
        if self.config.action_feature is not None:
            self.config.action_dim = self.config.action_feature.shape[0]

    def get_optim_params(self):
        return self.parameters()

    def reset(self):
        self._action_queue: deque[Tensor] = deque([], maxlen=self.config.n_action_steps)
        self._rtc_served = 0      # actions served since the last plan: the shift of the next guided one
        if getattr(self, "model", None) is not None:
            self.model.rtc_reset()      # (rtc: the next plan of every environment is unguided)
        if getattr(self, "_ensembler", None) is not None:
            self._ensembler.close()
            self._ensembler = None

    def enable_image_augmentation(self, **kwargs):
        """image augmentation of training batches: the backbone's state, as vla_fastvlm.fastvla.FastVLAPolicy.enable_image_augmentation sets it"""
        return self.model.backbone.enable_image_augmentation(**kwargs)

    def disable_image_augmentation(self) -> None:
        self.model.backbone.disable_image_augmentation()

    def fold_dataset_stats(self, dataset_stats) -> None:
        """Take over the STATE / ACTION MEAN_STD normalisation LeRobot's processors would apply around the policy
        (reference lerobot_fastvla/processor_fastvla.py:34-48 with the map of configuration_fastvla.py:21-27): raw states go
        in, un-normalised actions come out of `select_action`, with the arithmetic folded into the head kernels.
        `forward(batch)` still expects NORMALISED action targets (the loss lives in normalised space).  None switches it off."""
        if dataset_stats is None:
            self.model.backbone.set_io_normalization()
            return
        act_key = next((k for k, ft in (self.config.output_features or {}).items() if ft.type is FeatureType.ACTION), ACTION)
        st, ac = dataset_stats[self._state_key], dataset_stats[act_key]
        self.model.backbone.set_io_normalization(state_mean=st["mean"], state_std=st["std"], action_mean=ac["mean"], action_std=ac["std"])

    def _prepare_inputs(self, batch: dict[str, Tensor]) -> tuple[Tensor, Tensor, list[str]]:
        images = batch[self._image_keys[0]]  # only the first camera feeds the backbone
        if images.ndim == 5:
            images = images[:, -1]
        states = batch[self._state_key]
        if states.ndim == 3:
            states = states[:, -1]
        n = images.shape[0]
        task = batch.get("task")
        if task is None:
            tasks = [""] * n
        elif isinstance(task, (list, tuple)):
            tasks = [str(t) for t in task]
            tasks = tasks * n if len(tasks) == 1 and n > 1 else tasks
        else:
            tasks = [str(task)] * n
        if self.config.add_trailing_newline:
            tasks = [t if t.endswith("\n") else t + "\n" for t in tasks]
        return images, states, tasks

    def _predict_actions(self, batch: dict[str, Tensor]) -> Tensor:
        images, states, tasks = self._prepare_inputs(batch)
        return self.model(images, states, tasks, device=images.device)

    def _coherent_plan(self, batch, *, shift: int) -> Tensor:
        """flow_select="coherent" without rtc: the candidate that best continues the chunks planned last (read `shift` steps ahead), for all B environments"""
        images, states, tasks = self._prepare_inputs(batch)
        pooled = self.model.features(images, tasks, device=images.device)
        chunk = self.model.sample_multi(pooled, states, shift=shift)
        self._rtc_served = 0
        return chunk if chunk.ndim == 3 else chunk.unsqueeze(1)

    @torch.no_grad()
    def predict_action_chunk(self, batch: dict[str, Tensor], inference_delay=None, prev_chunk_left_over=None, execution_horizon=None, num_samples=None,
                             **kwargs) -> Tensor:
        """rtc (LeRobot's keyword set, for all B environments in one call): prev_chunk_left_over (B, K', A), K' <= K, the not-yet-executed rows of the
        previous chunk in normalised space (last_chunk_normalised[:, executed:]); inference_delay d: its first d steps are a hard prefix; execution_horizon:
        the last steps left free (default: the policy's).  Without prev_chunk_left_over the plan is guided by the chunk planned last, from its start
        (none after reset(): unguided).
        num_samples (flow_samples > 1; 1 .. flow_samples): the candidates of THIS call; the chosen chunk of every environment is returned."""
        if num_samples is not None:
            from fastvla_hip.select import check_flow_samples
            if check_flow_samples(num_samples) > self.flow_samples:
                raise ValueError(f"num_samples={num_samples} exceeds the flow_samples={self.flow_samples} the policy was constructed with (the sampler's rows are sized for it)")
            self.model.flow_samples_now = int(num_samples)
            try:
                return self.predict_action_chunk(batch, inference_delay=inference_delay, prev_chunk_left_over=prev_chunk_left_over, execution_horizon=execution_horizon)
            finally:
                self.model.flow_samples_now = self.flow_samples
        self.eval()
        if self.rtc is None and self.flow_select == "coherent":
            if inference_delay or prev_chunk_left_over is not None or execution_horizon is not None:
                raise ValueError(f"inference_delay / prev_chunk_left_over / execution_horizon need rtc=True. Got inference_delay={inference_delay}, rtc=False.")
            return self._coherent_plan(batch, shift=0)
        if self.rtc is None:
            if inference_delay or prev_chunk_left_over is not None or execution_horizon is not None:
                raise ValueError(f"inference_delay / prev_chunk_left_over / execution_horizon need rtc=True. Got inference_delay={inference_delay}, rtc=False.")
            actions = self._predict_actions(batch)
            return actions if actions.ndim == 3 else actions.unsqueeze(1)  # [B, chunk_size, A]
        K, A = self.model.chunk_size, self.config.action_dim
        prev, shift = None, 0
        if prev_chunk_left_over is not None:
            rows = torch.as_tensor(prev_chunk_left_over, dtype=torch.float32)
            if rows.ndim != 3 or rows.shape[2] != A or not 1 <= rows.shape[1] <= K:
                raise ValueError(f"prev_chunk_left_over must be (B, 1 .. {K}, {A}), got {tuple(rows.shape)}")
            shift = K - rows.shape[1]
            prev = torch.zeros(rows.shape[0], K, A, dtype=torch.float32, device=rows.device)
            prev[:, shift:] = rows
        # (inference_delay None: 0 under rtc_method="guidance", the policy's rtc_prefix_steps under "prefix" -- FastVLMWithExpert.rtc_sample's default)
        return self._rtc_plan(batch, shift=shift, inference_delay=None if inference_delay is None else int(inference_delay), execution_horizon=execution_horizon,
                              prev=prev)

    def _rtc_plan(self, batch, *, shift: int, inference_delay=None, execution_horizon=None, prev=None) -> Tensor:
        images, states, tasks = self._prepare_inputs(batch)
        pooled = self.model.features(images, tasks, device=images.device)
        chunk = self.model.rtc_sample(pooled, states, shift=shift, inference_delay=inference_delay, execution_horizon=execution_horizon, prev=prev)
        self._rtc_served = 0
        return chunk

    @torch.no_grad()
    def select_action(self, batch: dict[str, Tensor]) -> Tensor:
        self.eval()
        if self.temporal_ensemble_coeff is not None:      # the backbone on every call; all B environments ensembled in one launch
            chunk = self.predict_action_chunk(batch)
            B, eng, ens = chunk.shape[0], self.model._engine(), self._ensembler
            if ens is not None and ens._engine is eng and ens._h and ens.n_env != B:
                raise ValueError(f"select_action: the batch holds {B} environments, the temporal ensembler was started with {ens.n_env}: call reset() first")
            if ens is None or ens._engine is not eng or not ens._h:
                from fastvla_hip.ensemble import TemporalEnsembler
                ens = self._ensembler = TemporalEnsembler(eng, B, self.model.chunk_size, self.config.action_dim, self.temporal_ensemble_coeff)
            return ens.step(chunk)
        if self.rtc is not None:
            if not self._action_queue:      # guided by the chunks planned last, read from the first step that has not been served yet
                self._action_queue.extend(self._rtc_plan(batch, shift=self._rtc_served)[:, : self.config.n_action_steps].transpose(0, 1))
            self._rtc_served += 1
            return self._action_queue.popleft()
        if self.flow_select == "coherent":      # (without rtc: the re-plan best continues the chunks planned last from the first step not served yet)
            if not self._action_queue:
                self._action_queue.extend(self._coherent_plan(batch, shift=min(self._rtc_served, self.model.chunk_size))[:, : self.config.n_action_steps].transpose(0, 1))
            self._rtc_served += 1
            return self._action_queue.popleft()
        if not self._action_queue:
            chunk = self.predict_action_chunk(batch)[:, : self.config.n_action_steps]
            self._action_queue.extend(chunk.transpose(0, 1))
        return self._action_queue.popleft()

    def forward(self, batch: dict[str, Tensor]) -> tuple[Tensor, dict]:
        images, states, tasks = self._prepare_inputs(batch)
        # head forward + loss (+ the head gradients autograd will ask for) in one pass through the library
        # chunk_size = 1: the one target is delta index 0, the observation's own frame, which never lies past the episode end -- the (B, 1) action_is_pad
        # every LeRobot dataset delivers is all False there and is not passed on, so default training stays on the plain MSE kernel and keeps its bits
        pad = batch.get("action_is_pad") if self.model.chunk_size > 1 else None
        loss, _pred = self.model.forward_loss(images, states, tasks, batch[ACTION], device=images.device, pad=pad)
        val = loss.item()
        met = self.model.last_loss_metrics      # the chunked loss kernel's masked MSE; None on the plain MSE path, where the loss IS the MSE
        info = {"loss": val, "mse": val if met is None else met[0].item()}
        if self.model.bins is not None:      # a binned head: the loss is a cross-entropy, "mse" the decoded chunk's, and the bin accuracy joins them
            info["accuracy"] = met[2].item()
        return loss, info
