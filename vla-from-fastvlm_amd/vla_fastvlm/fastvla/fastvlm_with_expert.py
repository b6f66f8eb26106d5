"""FastVLM backbone + action-expert head (reference: src/vla_fastvlm/fastvla/fastvlm_with_expert.py:12-54).

The module tree (`state_projection`, `fusion`, `action_head`) and therefore the state-dict keys are the reference's;
the 12 trainable tensors are views into ONE flat fp32 device buffer so the HIP head kernels, the fused AdamW and the
RCCL all-reduce each see a single contiguous array, while `parameters()`, `state_dict()` and any torch optimizer keep
working on the same nn.Parameters.  forward/backward of the head run in libfastvla_hip.so via one autograd.Function.
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn

from fastvla_hip import HEAD_KEYS

from ..model.fastvlm_adapter import FastVLMBackbone
from .configuration_fastvla import FastVLAConfig
from .options import PolicyOptions


class _HeadFunction(torch.autograd.Function):
    """actions = head(pooled, states); backward hands dL/dactions to fv_head_backward and returns views of the flat
    gradient buffer for the 12 parameters (the frozen backbone and the states get no gradient)."""

    @staticmethod
    def forward(ctx, owner, pooled, states, training, differentiable, *params):
        eng, flat = owner._engine(), owner._flat
        p = float(owner.config.dropout) if training else 0.0
        owner._drop_calls += 1
        # `differentiable` (a gradient may be asked of these actions, in train OR eval mode): keep them in normalised space --
        # fv_head_backward differentiates the head, not the folded `* action_std + action_mean` behind it
        actions, saved = eng.head_forward(flat, pooled, states, training=bool(training and p > 0.0), dropout_p=p,
                                          seed=owner._drop_seed, offset=owner._drop_calls,
                                          normalized_actions=bool(training or differentiable))
        ctx.owner, ctx.saved, ctx.p = owner, saved, p
        return actions

    @staticmethod
    def backward(ctx, grad_actions):
        owner = ctx.owner
        grads = owner._engine().head_backward_from_grad(owner._flat, grad_actions, ctx.saved, ctx.p)
        views = owner._engine().head_views(grads)
        return (None, None, None, None, None) + tuple(views[k] for k in HEAD_KEYS)


class _HeadLossFunction(torch.autograd.Function):
    """(loss, actions) = (mse(head(pooled, states), targets), head(...)) with the head forward, the MSE and the head
    backward all inside libfastvla_hip.so (fv_head_forward + fv_head_mse_backward): what the reference spells as
    `F.mse_loss(pred, target)` + autograd (fastvla/modeling_fastvla.py:56, lerobot_fastvla/modeling_fastvla.py:132).
    backward() only scales the flat gradient by the incoming dL/dloss (fv_grad_scale) and hands out views of it."""

    @staticmethod
    def forward(ctx, owner, pooled, states, targets, pad, training, *params):
        eng, flat = owner._engine(), owner._flat
        p = float(owner.config.dropout) if training else 0.0
        owner._drop_calls += 1
        actions, saved = eng.head_forward(flat, pooled, states, training=bool(training and p > 0.0), dropout_p=p,
                                          seed=owner._drop_seed, offset=owner._drop_calls, normalized_actions=True)  # a loss: normalised space
        loss, grads = eng.head_backward(flat, actions, targets, saved, dropout_p=p, pad=pad)
        # the chunked loss kernel also reports the masked MSE and the valid fraction; the plain MSE path has nothing beside its loss
        owner.last_loss_metrics = eng.head_loss_metrics() if eng.loss_is_chunked(pad) else None
        ctx.owner, ctx.grads = owner, grads
        ctx.mark_non_differentiable(actions)
        return loss[0], actions

    @staticmethod
    def backward(ctx, grad_loss, _grad_actions):
        eng = ctx.owner._engine()
        eng.grad_scale(ctx.grads, grad_loss.reshape(1).to(ctx.grads.device, torch.float32).contiguous())
        views = eng.head_views(ctx.grads)
        return (None, None, None, None, None, None) + tuple(views[k] for k in HEAD_KEYS)


class _FlowLossFunction(torch.autograd.Function):
    """_HeadLossFunction for the flow head: fv_head_flow_prepare noises the targets (x_t and phi(t) go straight into the saved activations, u = eps - a comes
    back), the head predicts the velocity and the configured loss compares it with u -- prepare, forward, loss and backward all inside the library.  The
    second output is the predicted VELOCITY, in normalised space."""

    @staticmethod
    def forward(ctx, owner, pooled, states, targets, pad, training, *params):
        eng, flat = owner._engine(), owner._flat
        p = float(owner.config.dropout) if training else 0.0
        owner._drop_calls += 1
        saved = eng.head_saved(pooled.shape[0])
        seed, offset = owner.flow_loss_draw() if training else owner.flow_eval_draw()
        u = eng.head_flow_prepare(targets, saved, seed=seed, offset=offset)
        v, saved = eng.head_forward(flat, pooled, states, training=bool(training and p > 0.0), dropout_p=p, seed=owner._drop_seed, offset=owner._drop_calls,
                                    saved=saved, normalized_actions=True)
        loss, grads = eng.head_backward(flat, v, u, saved, dropout_p=p, pad=pad)
        owner.last_loss_metrics = eng.head_loss_metrics() if eng.loss_is_chunked(pad) else None
        ctx.owner, ctx.grads = owner, grads
        v = v[:pooled.shape[0]]      # flow_noise_draws > 1: u and v hold every draw's rows (draw-major); the loss is the S-draw loss, the velocity handed out draw 0's
        ctx.mark_non_differentiable(v)
        return loss[0], v

    @staticmethod
    def backward(ctx, grad_loss, _grad_actions):
        eng = ctx.owner._engine()
        eng.grad_scale(ctx.grads, grad_loss.reshape(1).to(ctx.grads.device, torch.float32).contiguous())
        views = eng.head_views(ctx.grads)
        return (None, None, None, None, None, None) + tuple(views[k] for k in HEAD_KEYS)


class FastVLMWithExpert(nn.Module):
    def __init__(self, config: FastVLAConfig, options: Optional[PolicyOptions] = None) -> None:
        """options: fastvla.options.resolve_policy_options' result (None: the defaults, the reference's model).  What the head takes from it --
        chunk["chunk_size"] = K > 1 (an extension of this build; the pinned core config has no such field): the head predicts K future steps per observation --
        `action_head` is Linear(fusion_dim, K * A), actions are (B, K, A).  chunk["loss"]: "mse" | "l1" | "smooth_l1" (beta), evaluated inside the library.
        flow = FastVLAEngine.set_head_flow's keyword arguments: the flow-matching head -- fusion.0 reads K * A + time_dim more columns (x_t and phi(t)),
        head() samples with flow_steps steps of the solver, head_loss() noises its targets and returns the predicted velocity.  flow_seed: the noise streams' seed
        (default: torch's initial seed, as the dropout stream's).  noise_draws = S (1 .. 16): S noise draws (t, eps) per observation wherever targets are
        noised -- draw s of a call at offset o is the single draw of offset o + (s << 56); the velocity handed out is draw 0's.
        prefix = fastvla_hip.prefix.check_prefix_config's result (flow head, K > 1): action-prefix conditioning -- fusion.0 reads K mask columns behind
        phi(t), training gives the first d <= max_delay steps of a chunk to the network clean and keeps them out of the loss, rtc_sample pins them.
        solver: "euler" | "midpoint" | "heun" | "rk4", the integrator of every sampling route (flow_steps are steps of it); a property of the run.
        samples = S (1 .. 16) with select "first" | "medoid" | "coherent" (fastvla_hip/select.py): every sampling route draws S candidates per
        observation in one call and returns the chosen one; "coherent" weights step k of the overlap with the previous chunk decay**k.
        A property of the run; S = 1 calls nothing new.
        bins = FastVLAEngine.set_head_bins' keyword arguments: the binned head -- `action_head` is Linear(fusion_dim, K * A * bins), head() returns the DECODED
        chunk, head_loss() the cross-entropy of the logits against the binned targets beside it, action_bin_probs() the per-element distributions.
        The cross-field refusals are HeadSpec's (fastvla_hip/head_spec.py)."""
        super().__init__()
        from fastvla_hip.head_spec import HeadSpec
        from fastvla_hip.select import check_flow_select, coherence_weights
        o = PolicyOptions() if options is None else options
        K = o.chunk["chunk_size"]
        # (the one pair checked here and not in HeadSpec, which holds no select name: a hand-built PolicyOptions gets its "medoid" default and a refusal
        # that names the select it asked for)
        self.flow_samples, self.flow_select = check_flow_select(o.samples, o.select, action_head="flow" if o.flow is not None else "regression", chunk_size=K)
        self.flow_samples_now = self.flow_samples      # select_action_chunk(num_samples=) lowers it for one call
        self.last_candidates = self.last_choice = self.last_sample_spread = None      # device tensors of the last multi-sample call
        self._coherence_weights = coherence_weights(int(K), o.decay) if self.flow_select == "coherent" else None
        spec = HeadSpec(dims=dict(state_dim=config.state_dim, action_dim=K * config.action_dim, hidden_dim=config.hidden_dim, fusion_dim=config.fusion_dim),
                        loss=dict(kind=o.chunk["loss"], beta=o.chunk["beta"], chunk=K), flow=None if o.flow is None else dict(o.flow),
                        flow_time=None if o.flow_time is None else dict(o.flow_time), prefix=None if o.prefix is None else dict(o.prefix), draws=o.noise_draws, solver=o.solver,
                        samples=dict(max_samples=self.flow_samples, step_weights=self._coherence_weights) if self.flow_samples > 1 else None,
                        bins=None if o.bins is None else dict(o.bins))
        self.config = config
        self.flow_noise_draws = spec.draws
        self.action_loss, self.action_loss_beta, self.chunk_size = spec.loss["kind"], spec.loss["beta"], spec.loss["chunk"]
        self.head_width = self.chunk_size * config.action_dim
        self.last_loss_metrics: Optional[torch.Tensor] = None    # (2,) [masked MSE, valid fraction] of the last loss the chunked kernel evaluated, else None
                                                                 # (a binned head: (3,), + the fraction of valid elements whose most likely bin is the target's)
        self.backbone = FastVLMBackbone(config.to_backbone_config())
        self.backbone.configure_head(spec)
        self.flow, self.flow_prefix, self.flow_steps = spec.flow, spec.prefix, int(o.flow_steps)
        self.bins = spec.bins      # the binned head's {"bins", "range", "sigma", "decode"}; None: another head
        self.flow_time = spec.flow_time      # the training time beyond set_head_flow's own distribution (flow_time_dist "beta:..." | "pi0", range, strata); None: off
        self._flow_solver = spec.solver
        self._flow_solver_rows = spec.solver_rows      # a policy built with a higher-order solver reserved their rows and may switch among all four
        self.rtc: Optional[dict] = None      # configure_rtc: real-time chunking of the flow sampler, a property of the run
        self._chunker = self._rtc_key = None
        extra = self.head_width + int(self.flow["time_dim"]) + (self.chunk_size if self.flow_prefix else 0) if self.flow else 0
        # same module tree / init as the reference so checkpoints and seeds line up
        self.state_projection = nn.Sequential(nn.LayerNorm(config.state_dim), nn.Linear(config.state_dim, config.hidden_dim), nn.SiLU())
        self.fusion = nn.Sequential(
            nn.Linear(self.backbone.output_dim + config.hidden_dim + extra, config.fusion_dim), nn.LayerNorm(config.fusion_dim),
            nn.SiLU(), nn.Dropout(config.dropout), nn.Linear(config.fusion_dim, config.fusion_dim), nn.SiLU())
        self.action_head = nn.Linear(config.fusion_dim, self.head_width * (self.bins["bins"] if self.bins else 1))
        self._flat: Optional[torch.Tensor] = None
        self._drop_seed = int(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
        self._drop_calls = 0
        self._flow_seed = int(self._drop_seed if o.flow_seed is None else o.flow_seed) & 0x7FFFFFFFFFFFFFFF
        self._flow_loss_calls = self._flow_eval_index = self._flow_sample_calls = 0
        if o.chunk["dim_weights"] is not None or o.chunk["step_weights"] is not None:
            self.set_action_loss_weights(o.chunk["dim_weights"], o.chunk["step_weights"])
        if o.rtc is not None:
            self.configure_rtc(o.rtc)

    # ------------------------------------------------------------------ flow head: the noise streams.  ONE seed, four disjoint offset ranges
    def flow_train_draw(self, step: int, micro: int):
        """(seed, offset) of a train step's noising: a function of the optimiser step, the micro-batch inside it and the data-parallel rank -- a resumed run
        continues the stream, and replicas that share one seed still draw different t and eps for their local row b (the noise batch is B * world, not B)"""
        import torch.distributed as dist
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return self._flow_seed, self.flow_train_offset(rank, step, micro)

    @staticmethod
    def flow_train_offset(rank: int, step: int, micro: int) -> int:
        """the offset layout of a train step: micro-batch bits 0 .. 15, optimiser step 16 .. 43, rank 44 .. 55.  Bits 56 .. 59 number the noise draws
        (flow_noise_draws: draw s draws at offset + (s << 56)) and bits 60 .. 62 mark the compute_loss / eval / sampling ranges, so a rank >= 4096 would
        run into them: ValueError"""
        if not 0 <= int(rank) < 4096:
            raise ValueError(f"flow_train_draw: rank {rank} outside 0 .. 4095 (the rank takes bits 44 .. 55 of the noise offset; 56 .. 59 number the draws)")
        return (int(rank) << 44) + (int(step) << 16) + (int(micro) & 0xFFFF)

    def flow_loss_draw(self):
        """compute_loss / forward(batch) in train() mode, outside the native train step: a running counter"""
        self._flow_loss_calls += 1
        return self._flow_seed, (1 << 60) + self._flow_loss_calls

    def flow_eval_draw(self):
        """eval() mode: a function of the evaluation batch index, which restarts whenever the module's mode is set (Trainer.evaluate calls eval() first) --
        two evaluations of the same weights see the same noise and give the same loss"""
        self._flow_eval_index += 1
        return self._flow_seed, (1 << 61) + self._flow_eval_index

    def flow_sample_draw(self):
        """predict / select_action: advances per call"""
        self._flow_sample_calls += 1
        return self._flow_seed, (1 << 62) + self._flow_sample_calls

    def train(self, mode: bool = True):
        self._flow_eval_index = 0
        return super().train(mode)

    def flow_error_draw(self):
        """action_error_per_dim: ONE fixed offset in a range of its own (bit 63) -- two calls sample from the same noise, and no counter advances"""
        return self._flow_seed, 1 << 63

    def flow_time_loss_draw(self):
        """flow_loss_per_time: ONE fixed offset in a range of its own (bits 62 and 63 both set; the draw bits 56 .. 59 stay free) -- two calls see the same
        noise, and no counter advances"""
        return self._flow_seed, (1 << 63) | (1 << 62)

    @property
    def flow_solver(self) -> str:
        """"euler" | "midpoint" | "heun" | "rk4": the integrator of every sampling route"""
        return self._flow_solver

    @flow_solver.setter
    def flow_solver(self, name: str) -> None:
        from fastvla_hip.engine import check_flow_solver
        name = check_flow_solver(name)
        if self.flow is None:
            raise ValueError(f"flow_solver={name!r} needs action_head='flow' (the regression head integrates nothing)")
        if name != "euler" and not self._flow_solver_rows:
            raise ValueError(f"flow_solver={name!r}: this policy was built with flow_solver='euler', so the two rows a higher-order solver works over were "
                             "not reserved in the workspace -- build the policy with flow_solver='midpoint' | 'heun' | 'rk4' (or FASTVLA_FLOW_SOLVER); it may "
                             "then switch among all four at any time")
        self.backbone.configure_head_flow_solver(name)
        self._flow_solver = name

    def flow_record(self) -> Optional[dict]:
        """hip_extras.json "action_head": there only in flow mode ("solver" only when it is not Euler: an Euler run writes the record it wrote) and for a
        binned head ({"type": "bins", "bins", "range", "sigma", "decode"})"""
        if self.bins is not None:
            return {"type": "bins", "bins": int(self.bins["bins"]), "range": [[float(lo), float(hi)] for lo, hi in self.bins["range"]], "sigma": float(self.bins["sigma"]),
                    "decode": self.bins["decode"]}
        if self.flow is None:
            return None
        from fastvla_hip import prefix as _prefix
        rec = {"type": "flow", "steps": int(self.flow_steps), **{k: self.flow[k] for k in ("time_dim", "min_period", "max_period", "time_dist", "dist_a", "dist_b")},
               "seed": int(self._flow_seed), **_prefix.extras_record(self.flow_prefix)}
        if self._flow_solver != "euler":
            rec["solver"] = self._flow_solver
        if self.flow_time is not None:      # "time_dist" holds the string; "time_range" / "time_stratify" only when set; dist_a / dist_b keep their constants
            tm = self.flow_time
            rec["time_dist"] = tm["name"]
            if (tm["t_lo"], tm["t_hi"]) != (0.0, 1.0):
                rec["time_range"] = [tm["t_lo"], tm["t_hi"]]
            if tm["stratify"]:
                rec["time_stratify"] = True
        return rec

    # ------------------------------------------------------------------ flat parameter storage
    def head_parameters(self):
        named = dict(self.named_parameters())
        return [named[k] for k in HEAD_KEYS]

    def _engine(self):
        return self.backbone.engine()

    def materialize(self, device: torch.device | None = None) -> torch.Tensor:
        """Move the 12 head tensors into one flat device buffer (idempotent) and re-point the Parameters at it."""
        eng = self.backbone.engine(device)
        params = self.head_parameters()
        views = None if self._flat is None else eng.head_views(self._flat)
        if views is not None and all(p.data_ptr() == views[k].data_ptr() for p, k in zip(params, HEAD_KEYS)):
            return self._flat
        flat = torch.zeros(eng.head_numel(), dtype=torch.float32, device=eng.device)
        views = eng.head_views(flat)
        with torch.no_grad():
            for p, k in zip(params, HEAD_KEYS):
                views[k].copy_(p.detach().to(eng.device, torch.float32))
                p.data = views[k]
        self._flat = flat
        return flat

    def flat_grads(self) -> Optional[torch.Tensor]:
        """The flat gradient buffer if every .grad is a view of one (true after a backward through _HeadFunction)."""
        params = self.head_parameters()
        if any(p.grad is None for p in params):
            return None
        base = params[0].grad._base if params[0].grad._base is not None else None
        if base is None or any(p.grad._base is not base for p in params):
            return None
        return base

    # ------------------------------------------------------------------ action chunks
    def set_action_loss(self, kind: str, beta: float = 1.0) -> None:
        """the loss of every later loss evaluation / train step: "mse" | "l1" | "smooth_l1" (beta)"""
        self.backbone.configure_head_loss(kind, beta, self.chunk_size)
        self.action_loss, self.action_loss_beta = self.backbone.head_spec.loss["kind"], self.backbone.head_spec.loss["beta"]

    def set_action_loss_weights(self, dim_weights=None, step_weights=None) -> None:
        """Weights of the loss of every later loss evaluation / train step: dim_weights (A values, e.g. gripper against arm) and step_weights (K values, e.g.
        a discount over the chunk); either may be None = ones, both None switches weighting off.  A weight of 0 takes the element out of the loss like a
        padded step.  ValueError for a wrong length or a negative / non-finite value."""
        self.backbone.configure_head_loss_weights(dim_weights, step_weights)

    @property
    def action_loss_weights(self) -> Optional[dict]:
        """{"dim": [A floats] or None, "step": [K floats] or None}, or None while weighting is off"""
        return self.backbone.head_spec.loss_weights

    def chunk_record(self, n_action_steps: int = 1, temporal_ensemble_coeff: Optional[float] = None) -> Optional[dict]:
        """what a checkpoint records beside the tensors (hip_extras.json "action_chunk"); None with the defaults.  "temporal_ensemble_coeff", "dim_weights" and
        "step_weights" are there only when set: every other policy's record is what it was."""
        rec = {"chunk_size": self.chunk_size, "n_action_steps": int(n_action_steps), "loss": self.action_loss, "beta": self.action_loss_beta}
        if temporal_ensemble_coeff is not None:
            rec["temporal_ensemble_coeff"] = float(temporal_ensemble_coeff)
        w = self.action_loss_weights or {}
        for key, name in (("dim", "dim_weights"), ("step", "step_weights")):
            if w.get(key) is not None:
                rec[name] = [float(x) for x in w[key]]
        return None if rec == {"chunk_size": 1, "n_action_steps": 1, "loss": "mse", "beta": 1.0} else rec

    def action_error_per_dim(self, pooled: torch.Tensor, states: torch.Tensor, targets: torch.Tensor, pad=None) -> torch.Tensor:
        """-> (A,): mean |prediction - target| over the non-padded steps of each action dimension, in the normalised space the loss lives in (what the
        per-dimension weights are tuned against); never weighted, no gradient.  A flow head SAMPLES one chunk per row with the policy's solver and step
        count, from the flow seed's noise at a fixed offset (flow_error_draw): two calls on the same weights agree bit for bit and the sampling counter
        does not advance -- the action-space metric a solver and a step count are chosen with.  (A prefix-width head samples with m = 0.)"""
        self.materialize(pooled.device)
        targets, pad = self.chunk_targets(targets.to(pooled.device, torch.float32), pad)
        if targets.shape != (pooled.shape[0], self.head_width):
            raise ValueError(f"targets must be (B,{self.config.action_dim}), got {tuple(targets.shape)}")
        eng = self._engine()
        if self.flow is not None:
            with torch.no_grad():
                seed, offset = self.flow_error_draw()
                # the prefix sampler with a delay of 0 everywhere: nothing pinned, m = 0, and chunk_out is the sample BEFORE the folded un-normalisation
                # (fv_head_flow_sample_prefix's pinned-step clamp selects; with p_b = 0 the previous chunk is never read)
                zeros = torch.zeros(pooled.shape[0], self.head_width, dtype=torch.float32, device=pooled.device)
                if self.flow_prefix is not None:
                    _, chunk = eng.head_flow_sample_prefix(self._flat, pooled, states.to(pooled.device, torch.float32), zeros,
                                                           torch.zeros(pooled.shape[0], dtype=torch.int32, device=pooled.device), steps=self.flow_steps, seed=seed,
                                                           offset=offset)
                else:
                    chunk = eng.head_flow_sample(self._flat, pooled, states.to(pooled.device, torch.float32), steps=self.flow_steps, seed=seed, offset=offset)
                    io = self.backbone._io_norm
                    if io is not None:      # the plain sampler hands out un-normalised actions only: undo the folded x std + mean (one rounding each way)
                        std = torch.as_tensor(io["action_std"], dtype=torch.float32, device=chunk.device).reshape(1, -1).repeat(1, self.chunk_size)
                        mean = torch.as_tensor(io["action_mean"], dtype=torch.float32, device=chunk.device).reshape(1, -1).repeat(1, self.chunk_size)
                        chunk = torch.where(std > 0, (chunk - mean) / std, torch.zeros_like(chunk))
                S = self.flow_noise_draws      # (the metric kernel counts head rows in draws: every draw sees the one sampled chunk)
                return eng.head_loss_per_dim(chunk.repeat(S, 1) if S > 1 else chunk, targets.repeat(S, 1) if S > 1 else targets.contiguous(), pad=pad)
        with torch.no_grad():
            actions, _saved = eng.head_forward(self._flat, pooled, states.to(pooled.device, torch.float32), normalized_actions=True)
            return eng.head_loss_per_dim(actions, targets.contiguous(), pad=pad)

    def flow_loss_per_time(self, pooled: torch.Tensor, states: torch.Tensor, targets: torch.Tensor, pad=None, buckets: int = 10):
        """-> (mse, count), each (buckets,) on the device: the velocity error as a function of t -- per time bucket the mean of (v - u)^2 over the non-padded
        elements of the head rows in it (0 where there is none) and their number; never weighted, whatever the loss kind, no gradient.  Head row r (S B of
        them with flow_noise_draws = S) is noised at the EXPLICIT time ((r mod buckets) + 0.5) / buckets, so every bucket is covered whatever the training
        distribution is, from the flow seed's noise at a fixed offset (flow_time_loss_draw): no dropout, no counter advances, and two calls on the same weights
        agree bit for bit.  The metric a time distribution is judged with, as action_error_per_dim is a solver's.  (A prefix-width head is given m = 0.)"""
        if self.flow is None:
            raise ValueError("flow_loss_per_time needs action_head='flow' (the regression head has no time)")
        self.materialize(pooled.device)
        targets, pad = self.chunk_targets(targets.to(pooled.device, torch.float32), pad)
        if targets.shape != (pooled.shape[0], self.head_width):
            raise ValueError(f"targets must be (B,{self.config.action_dim}), got {tuple(targets.shape)}")
        eng = self._engine()
        with torch.no_grad():
            B, nb = pooled.shape[0], int(buckets)
            R = B * self.flow_noise_draws
            t = ((torch.arange(R, device=pooled.device) % nb).to(torch.float32) + 0.5) / float(nb)
            seed, offset = self.flow_time_loss_draw()
            saved = eng.head_saved(B)
            delays = torch.zeros(R, dtype=torch.int32, device=pooled.device) if self.flow_prefix is not None else None
            u = eng.head_flow_prepare(targets.contiguous(), saved, seed=seed, offset=offset, t=t, delays=delays)
            v, _ = eng.head_forward(self._flat, pooled, states.to(pooled.device, torch.float32), saved=saved, normalized_actions=True)
            out = eng.head_loss_per_time(v, u, t, nb, pad=pad)
            return torch.where(out[:, 1] > 0, out[:, 0] / out[:, 1].clamp_min(1.0), torch.zeros_like(out[:, 0])), out[:, 1]

    def chunk_targets(self, targets: torch.Tensor, pad=None):
        """-> (targets flattened to (B, K * A), pad (B, K) bool or None).  Targets are (B, K, A); (B, A) only when K == 1 (where a longer (B, T, A) gives its
        step 0, as ever).  pad = LeRobot's action_is_pad: True where a chunk step lies past the episode end.  Idempotent: what it returned passes through."""
        K, A = self.chunk_size, self.config.action_dim
        steps = None
        if targets.ndim == 3:
            steps = targets.shape[1]
            if K == 1:
                targets = targets[:, 0]
            elif tuple(targets.shape[1:]) != (K, A):
                raise ValueError(f"targets must be (B, {K}, {A}), got {tuple(targets.shape)}")
            else:
                targets = targets.reshape(targets.shape[0], K * A)
        elif K > 1 and not (targets.ndim == 2 and targets.shape[1] == K * A):      # ((B, K * A): this function's own output)
            raise ValueError(f"targets must be (B, {K}, {A}) with chunk_size={K}, got {tuple(targets.shape)}")
        if pad is not None:
            pad = torch.as_tensor(pad)
            if K == 1 and pad.ndim == 2 and steps is not None and pad.shape[1] == steps:
                pad = pad[:, :1]
            if tuple(pad.shape) != (targets.shape[0], K):
                raise ValueError(f"action_is_pad must be (B, {K}), got {tuple(pad.shape)}")
            pad = pad != 0
        return targets, pad

    def _shape_actions(self, actions: torch.Tensor) -> torch.Tensor:
        return actions.view(actions.shape[0], self.chunk_size, self.config.action_dim) if self.chunk_size > 1 else actions

    # ------------------------------------------------------------------ forward
    def features(self, images, tasks: List[str], device=None) -> torch.Tensor:
        return self.backbone(images, tasks, device=device)

    def head(self, pooled: torch.Tensor, states: torch.Tensor) -> torch.Tensor:
        self.materialize(pooled.device)
        states = states.to(pooled.device, torch.float32)
        if states.ndim != 2 or states.shape[1] != self.config.state_dim:
            raise ValueError(f"states must be (B,{self.config.state_dim}), got {tuple(states.shape)}")
        params = self.head_parameters()
        differentiable = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if self.flow is not None:
            if differentiable:
                raise RuntimeError("the flow head samples its actions (Euler steps of the velocity field) and sampling is not differentiated: call predict / "
                                   "forward under torch.no_grad(), and train through compute_loss / forward(batch) / the train step")
            if self.flow_samples > 1:      # (a call without a previous chunk to continue: "coherent" rows take the medoid)
                return self.sample_multi(pooled, states)
            seed, offset = self.flow_sample_draw()
            return self._shape_actions(self._engine().head_flow_sample(self._flat, pooled, states, steps=self.flow_steps, seed=seed, offset=offset))
        if self.bins is not None:
            if differentiable:
                raise ValueError("action_head='bins' decodes its actions from the bins (argmax / mean of the centres) and the decode is not differentiated: call predict "
                                 "/ forward under torch.no_grad(), and train through compute_loss / forward(batch) / the train step. Got action_head='bins' with "
                                 "autograd enabled.")
            actions, _saved = self._engine().head_forward(self._flat, pooled, states)      # (inference form: the folded action statistics behind the decode)
            return self._shape_actions(actions)
        actions = _HeadFunction.apply(self, pooled, states, self.training, differentiable, *params)
        io = self.backbone._io_norm
        if differentiable and not self.training and io is not None:
            # eval mode with autograd on: the library kept the actions in normalised space (its backward differentiates the head, not
            # the folded statistics); finish `* action_std + action_mean` here, in torch, so that predict() returns the SAME space with
            # and without torch.no_grad() -- and the result stays differentiable
            std = torch.as_tensor(io["action_std"], dtype=torch.float32, device=actions.device).reshape(1, -1).repeat(1, self.chunk_size)
            mean = torch.as_tensor(io["action_mean"], dtype=torch.float32, device=actions.device).reshape(1, -1).repeat(1, self.chunk_size)
            actions = actions * std + mean
        return self._shape_actions(actions)

    def action_bin_probs(self, pooled: torch.Tensor, states: torch.Tensor) -> torch.Tensor:
        """-> (B, K, A, bins) on the device: the binned head's distribution over the bins of every action element (softmax of the logits, no dropout); its entropy
        is an uncertainty signal.  No gradient."""
        if self.bins is None:
            raise ValueError("action_bin_probs needs action_head='bins'")
        self.materialize(pooled.device)
        states = states.to(pooled.device, torch.float32)
        if states.ndim != 2 or states.shape[1] != self.config.state_dim:
            raise ValueError(f"states must be (B,{self.config.state_dim}), got {tuple(states.shape)}")
        with torch.no_grad():
            eng, B = self._engine(), pooled.shape[0]
            _actions, saved = eng.head_forward(self._flat, pooled, states)
            return eng.head_bins_probs(saved, B).view(B, self.chunk_size, self.config.action_dim, self.bins["bins"])

    # ------------------------------------------------------------------ several samples per observation, one chosen on the device
    def sample_multi(self, pooled: torch.Tensor, states: torch.Tensor, *, shift: Optional[int] = None, delay: Optional[int] = None,
                     prev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> (B, K, A): flow_samples_now candidates per row in ONE sampler call (fv_head_flow_sample_multi), the one flow_select names returned; the
        candidates (B, S, K, A), the choice (B) and the spread (B, K, A) stay on the device in last_candidates / last_choice / last_sample_spread.
        shift (None: a call on its own): the plan continues the chunker's kept chunk, read `shift` steps ahead -- "coherent" scores against it (rows without
        one take the medoid) and the chosen chunk is kept; delay: the candidates come from the prefix sampler and pin their first steps to it."""
        self.materialize(pooled.device)
        states = states.to(pooled.device, torch.float32)
        if states.ndim != 2 or states.shape[1] != self.config.state_dim:
            raise ValueError(f"states must be (B,{self.config.state_dim}), got {tuple(states.shape)}")
        B, S, K, A = pooled.shape[0], int(self.flow_samples_now), self.chunk_size, self.config.action_dim
        seed, offset = self.flow_sample_draw()
        kw = dict(samples=S, steps=self.flow_steps, seed=seed, offset=offset)
        if shift is None:
            out = self._engine().head_flow_sample_multi(self._flat, pooled, states, select="medoid" if self.flow_select == "coherent" else self.flow_select, **kw)
        else:
            out = self._rtc_chunker(B).sample_multi(self._flat, pooled, states, select=self.flow_select, shift=int(shift), delay=delay, prev=prev, **kw)
        self.last_candidates = out["candidates"].view(S, B, K, A).transpose(0, 1)
        self.last_choice, self.last_sample_spread = out["choice"], out["spread"].view(B, K, A)
        return self._shape_actions(out["actions"])

    # ------------------------------------------------------------------ real-time chunking (flow head): the guided sampler
    def configure_rtc(self, rtc: Optional[dict]) -> None:
        """rtc = {"schedule", "max_guidance_weight", "execution_horizon"} (options.resolve_rtc_options) or None.  A property of the run: no checkpoint
        records it.  The weights of (inference_delay 0, execution_horizon) are handed to the backbone so that the engine is configured BEFORE its first
        workspace exists; another delay or horizon re-uploads them at the call that asks for it."""
        from fastvla_hip.rtc import prefix_weights
        if rtc is not None and rtc.get("method") != "prefix" and getattr(self, "flow_samples", 1) > 1:
            raise ValueError(f"flow_samples={self.flow_samples} with rtc_method='guidance': guided sampling with candidates is not offered")
        self.rtc = None if rtc is None else dict(rtc)
        self._chunker = None
        if rtc is not None and rtc.get("method") == "prefix":      # the prefix sampler: no guidance, no weights, nothing to configure on the engine
            if self.flow_prefix is None:
                raise ValueError("rtc_method='prefix' needs a head trained with flow_prefix_max_delay")
            self._rtc_key = None
            self.backbone.configure_head_flow_guidance(None)
            return
        self._rtc_key = None if rtc is None else (0, int(rtc["execution_horizon"]))
        self.backbone.configure_head_flow_guidance(
            None if rtc is None else dict(step_weights=prefix_weights(self.chunk_size, 0, rtc["execution_horizon"], rtc["schedule"]),
                                          max_guidance_weight=rtc["max_guidance_weight"]))

    def _rtc_chunker(self, n_env: int):
        from fastvla_hip.rtc import RealTimeChunker
        eng, ck = self._engine(), getattr(self, "_chunker", None)
        if ck is not None and ck._engine is eng and ck.n_env != n_env:
            raise ValueError(f"real-time chunking: the batch holds {n_env} environments, the previous chunks were kept for {ck.n_env}: call reset() first")
        if ck is None or ck._engine is not eng:      # (the first call after construction, or the engine was rebuilt underneath)
            fresh = ck is not None      # (a rebuilt engine holds the weights the backbone configured it with: delay 0, the policy's horizon)
            ck = self._chunker = RealTimeChunker(eng, n_env)
            if fresh and self.rtc is not None and self.rtc.get("method") != "prefix":
                self._rtc_key = (0, int(self.rtc["execution_horizon"]))
        return ck

    def rtc_reset(self, env: Optional[int] = None) -> None:
        """forget the previous chunk of one environment or of all: their next plan is unguided (a stream-ordered memset of the row mask)"""
        if getattr(self, "_chunker", None) is not None:
            self._chunker.reset(env)

    @property
    def last_chunk_normalised(self) -> Optional[torch.Tensor]:
        """(B, K, A) copy of the chunks the last guided call produced, in normalised space (what a later call takes as prev_chunk); None before the first"""
        ck = getattr(self, "_chunker", None)
        return None if ck is None else ck.prev.view(ck.n_env, self.chunk_size, self.config.action_dim).clone()

    def rtc_sample(self, pooled: torch.Tensor, states: torch.Tensor, *, shift: int = 0, inference_delay: Optional[int] = None,
                   execution_horizon: Optional[int] = None, prev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> (B, K, A): the flow sampler guided by the previous chunk read `shift` steps ahead -- the chunker's own (rows without one are sampled unguided),
        or `prev` (B, K, A) / (B, K * A), normalised, for every row.  rtc_method="prefix": the prefix sampler instead -- the first
        min(inference_delay, max_delay, K - shift) steps are PINNED to the previous chunk (inference_delay None: the policy's rtc_prefix_steps)."""
        from fastvla_hip.rtc import check_rtc, prefix_weights
        if getattr(self, "rtc", None) is None:
            raise RuntimeError("real-time chunking is off: construct the policy with rtc=True")
        self.materialize(pooled.device)
        states = states.to(pooled.device, torch.float32)
        if states.ndim != 2 or states.shape[1] != self.config.state_dim:
            raise ValueError(f"states must be (B,{self.config.state_dim}), got {tuple(states.shape)}")
        K = self.chunk_size
        if isinstance(shift, bool) or int(shift) != shift or not 0 <= int(shift) <= K:
            raise ValueError(f"shift must be an integer in 0 .. chunk_size = {K}, got {shift!r}")
        if self.rtc.get("method") == "prefix":
            from fastvla_hip.prefix import check_inference_delay
            if execution_horizon is not None:
                raise ValueError(f"execution_horizon belongs to rtc_method='guidance'. Got execution_horizon={execution_horizon}, rtc_method='prefix'.")
            d = self.rtc["prefix_steps"] if inference_delay is None else check_inference_delay(inference_delay, self.flow_prefix["max_delay"])
            ck = self._rtc_chunker(pooled.shape[0])
            if prev is not None:
                prev = prev.to(pooled.device, torch.float32).reshape(pooled.shape[0], -1)
                if prev.shape[1] != self.head_width:
                    raise ValueError(f"prev_chunk must hold (B, {K}, {self.config.action_dim}) elements, got {tuple(prev.shape)}")
            if self.flow_samples > 1:
                return self.sample_multi(pooled, states, shift=int(shift), delay=d, prev=prev)
            seed, offset = self.flow_sample_draw()
            return self._shape_actions(ck.sample_prefix(self._flat, pooled, states, shift=int(shift), delay=d, steps=self.flow_steps, seed=seed, offset=offset,
                                                        prev=prev))
        s = self.rtc["execution_horizon"] if execution_horizon is None else execution_horizon
        _, d, s = check_rtc(K, 0 if inference_delay is None else inference_delay, s, self.rtc["schedule"])
        ck = self._rtc_chunker(pooled.shape[0])
        if (d, s) != self._rtc_key:      # (a configuration call: it synchronises the device)
            self._engine().set_head_flow_guidance(prefix_weights(K, d, s, self.rtc["schedule"]), self.rtc["max_guidance_weight"])
            self._rtc_key = (d, s)
        if prev is not None:
            prev = prev.to(pooled.device, torch.float32).reshape(pooled.shape[0], -1)
            if prev.shape[1] != self.head_width:
                raise ValueError(f"prev_chunk must hold (B, {K}, {self.config.action_dim}) elements, got {tuple(prev.shape)}")
        seed, offset = self.flow_sample_draw()
        return self._shape_actions(ck.sample(self._flat, pooled, states, shift=int(shift), steps=self.flow_steps, seed=seed, offset=offset, prev=prev))

    def head_loss(self, pooled: torch.Tensor, states: torch.Tensor, targets: torch.Tensor, pad=None):
        """-> (loss 0-dim, actions): the loss (MSE unless set_action_loss chose another) of the head's prediction against `targets`, differentiable w.r.t.
        the 12 head tensors, with no torch operator between the pooled feature and the loss.  pad: optional (B, K) bool, True = the step does not train."""
        self.materialize(pooled.device)
        states = states.to(pooled.device, torch.float32)
        targets = targets.to(pooled.device, torch.float32).contiguous()
        if states.ndim != 2 or states.shape[1] != self.config.state_dim:
            raise ValueError(f"states must be (B,{self.config.state_dim}), got {tuple(states.shape)}")
        targets, pad = self.chunk_targets(targets, pad)
        if targets.shape != (pooled.shape[0], self.head_width):
            raise ValueError(f"targets must be (B,{self.config.action_dim}), got {tuple(targets.shape)}")
        fn = _HeadLossFunction if self.flow is None else _FlowLossFunction      # (flow: `actions` is the predicted velocity, in normalised space)
        loss, actions = fn.apply(self, pooled, states, targets.contiguous(), pad, self.training, *self.head_parameters())
        return loss, self._shape_actions(actions)

    def forward(self, images: torch.Tensor, states: torch.Tensor, tasks: List[str], device: torch.device | None = None) -> torch.Tensor:
        if device is None:
            device = images.device
        return self.head(self.features(images, tasks, device=device), states)

    def forward_loss(self, images, states, tasks: List[str], targets: torch.Tensor, device: torch.device | None = None, pad=None):
        """-> (loss, actions) for `compute_loss` / the LeRobot `forward(batch)`."""
        if device is None:
            device = images.device
        targets, pad = self.chunk_targets(targets, pad)     # (shape errors before the backbone runs)
        return self.head_loss(self.features(images, tasks, device=device), states, targets, pad)
