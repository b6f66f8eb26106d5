"""Everything an engine's action expert is configured with, in one record: FastVLMWithExpert builds it once, FastVLMBackbone keeps it and `apply` replays it
onto every engine it builds.  The cross-field refusals run at construction (and again whenever dataclasses.replace changes a field), from plain values: no
engine, no library call."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

# the fields an engine's head layout and workspaces are sized by, and the refusal a built engine answers a change of each with
LAYOUT_FIELDS = (("bins", "configure_head_bins: the engine is already built (the head's layout and the workspace depend on the mode)"),
                 ("flow", "configure_head_flow: the engine is already built (the head's layout and the workspace depend on the mode)"),
                 ("prefix", "configure_head_flow_prefix: the engine is already built (the head's layout and the workspace depend on the mode)"),
                 ("draws", "configure_head_flow_draws: the engine is already built (the saved activations and the workspaces depend on the number of draws)"),
                 ("samples", "configure_head_flow_samples: the engine is already built (the sampler's rows in the workspace depend on the number of samples)"))


@dataclass
class HeadSpec:
    dims: dict = field(default_factory=lambda: dict(state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024))      # FastVLAEngine's keywords; action_dim = K * A
    loss: dict = field(default_factory=lambda: dict(kind="mse", beta=1.0, chunk=1))      # set_head_loss' arguments: the fused loss and the chunk length K
    loss_weights: Optional[dict] = None      # {"dim", "step"} of the weighted chunk loss, None = off
    flow: Optional[dict] = None              # set_head_flow's arguments, None = the regression head
    bins: Optional[dict] = None              # set_head_bins' arguments {"bins", "range", "sigma", "decode"}, None = no binned head
    flow_time: Optional[dict] = None         # set_head_flow_time's arguments (+ "name", the checkpoint's string), None = set_head_flow's own distribution
    prefix: Optional[dict] = None            # fastvla_hip.prefix.check_prefix_config's record, None = off
    draws: int = 1                           # set_head_flow_draws' argument, 1 = one draw per observation
    guidance: Optional[dict] = None          # set_head_flow_guidance's arguments, None = off
    samples: Optional[dict] = None           # set_head_flow_samples' arguments, None = one sample
    solver: str = "euler"                    # set_head_flow_solver's argument
    solver_rows: bool = False                # a higher-order solver was named once: an engine is built with its two rows reserved

    def __post_init__(self):
        from .engine import check_flow_draws, check_flow_solver, check_flow_time, check_head_bins, check_head_loss, check_loss_weights
        from .prefix import check_prefix_config
        from .select import check_flow_select
        head = "regression" if self.flow is None else "flow"
        if self.bins is not None:
            if self.flow is not None:
                raise ValueError("action_head='bins' and the flow head exclude each other: got both action_bins and flow settings")
            if self.loss["kind"] != "mse":
                raise ValueError(f"action_head='bins' trains with its own cross-entropy: action_loss must stay 'mse', got action_loss={self.loss['kind']!r}")
            K = int(self.loss["chunk"])
            self.bins = check_head_bins(self.bins["bins"], self.bins["range"], self.bins["sigma"], self.bins["decode"], self.dims["action_dim"] // max(K, 1), K)
        # (the spec holds the samples' count and weights, not the select name: FastVLMWithExpert checks the pair, with the name, before it builds the spec)
        check_flow_select(None if self.samples is None else self.samples["max_samples"], None, action_head=head)
        self.draws = check_flow_draws(self.draws)
        if self.draws > 1 and self.flow is None:
            raise ValueError(f"flow_noise_draws={self.draws} needs action_head='flow' (the regression head has no noise to draw)")
        if self.flow_time is not None:
            tm = self.flow_time
            if self.flow is None:
                raise ValueError(f"flow_time_dist={tm.get('name', tm['dist'])!r} needs action_head='flow' (the regression head draws no time)")
            self.flow_time = dict(check_flow_time(tm["dist"], tm["a"], tm["b"], tm["t_lo"], tm["t_hi"], tm["stratify"]), name=str(tm.get("name", tm["dist"])))
            if self.flow_time["stratify"] and self.draws == 1:
                raise ValueError("flow_time_stratify=True needs flow_noise_draws > 1 (the strata are dealt to the draws of one observation), got flow_noise_draws=1")
        kind, beta, K = check_head_loss(self.loss["kind"], self.loss["beta"], self.loss["chunk"], self.dims["action_dim"])
        self.loss = dict(kind=kind, beta=beta, chunk=K)
        if self.loss_weights is not None:
            self.loss_weights = check_loss_weights(self.loss_weights["dim"], self.loss_weights["step"], self.dims["action_dim"] // K, K)
        if self.prefix is not None:
            if self.flow is None or int(self.prefix["chunk"]) != K:
                raise ValueError(f"flow_prefix_max_delay={self.prefix.get('max_delay')} needs action_head='flow' and the head's chunk_size={K}")
            check_prefix_config(self.prefix["max_delay"], action_head=head, chunk_size=K, dist=self.prefix["dist"], rate=self.prefix["rate"])
        self.solver = check_flow_solver(self.solver)
        if self.solver != "euler" and self.flow is None:
            raise ValueError(f"flow_solver={self.solver!r} needs action_head='flow' (the regression head integrates nothing)")
        self.solver_rows = bool(self.solver_rows or self.solver != "euler")      # (a policy switched back to Euler keeps its rows: it may switch again)

    def apply(self, engine) -> None:
        """Configure a NEW engine.  The order is a constraint of the library: flow mode first, the time distribution behind it (set_head_flow resets it);
        prefix, draws, guidance and samples before any workspace is bound; the solver twice, so that a spec switched back to Euler still reserves a higher-order solver's rows; switched-off options call nothing."""
        if self.bins is not None:
            engine.set_head_bins(**self.bins)
        if self.flow is not None:
            engine.set_head_flow(**self.flow)
            if self.flow_time is not None:
                engine.set_head_flow_time(**{k: v for k, v in self.flow_time.items() if k != "name"})
            if self.prefix is not None:
                px = self.prefix
                engine.set_head_flow_prefix(px["chunk"], px["max_delay"], thresholds=px["thresholds"], dist=px["dist"], rate=px["rate"])
            if self.draws > 1:
                engine.set_head_flow_draws(self.draws)
            if self.guidance is not None:
                engine.set_head_flow_guidance(**self.guidance)
            if self.samples is not None:
                engine.set_head_flow_samples(**self.samples)
            if self.solver_rows:
                engine.set_head_flow_solver(self.solver if self.solver != "euler" else "midpoint")
                engine.set_head_flow_solver(self.solver)
        if self.loss != dict(kind="mse", beta=1.0, chunk=1):
            engine.set_head_loss(**self.loss)
        if self.loss_weights is not None:
            engine.set_head_loss_weights(self.loss_weights["dim"], self.loss_weights["step"])
