"""What both policy surfaces hand through from FastVLMWithExpert (`self.model`) for a flow head: the sampler's settings and the last call's device tensors."""
from __future__ import annotations

from typing import Optional

import torch


class FlowSurfaceMixin:
    @property
    def flow_steps(self) -> int:
        """steps of the chosen solver (flow_solver) in a flow head's samplers (ignored by the regression head); may be changed at any time"""
        return self.model.flow_steps

    @flow_steps.setter
    def flow_steps(self, n: int) -> None:
        if int(n) != n or n < 1:
            raise ValueError(f"flow_steps must be an integer >= 1, got {n}")
        self.model.flow_steps = int(n)

    @property
    def flow_solver(self) -> str:
        """"euler" | "midpoint" | "heun" | "rk4": the integrator of every sampling route of a flow head.  A policy built with a higher-order solver may switch
        among all four at any time; one built with "euler" raises ValueError (the rows a higher-order solver works over were not reserved)"""
        return self.model.flow_solver

    @flow_solver.setter
    def flow_solver(self, name: str) -> None:
        self.model.flow_solver = name

    @property
    def last_candidates(self) -> Optional[torch.Tensor]:
        """flow_samples > 1: (B, S, K, A), the candidates of the last sampling call in normalised space, on the device; None before the first"""
        return self.model.last_candidates

    @property
    def last_choice(self) -> Optional[torch.Tensor]:
        """flow_samples > 1: (B) int32, the index of the candidate the last sampling call chose per row, on the device"""
        return self.model.last_choice

    @property
    def last_sample_spread(self) -> Optional[torch.Tensor]:
        """flow_samples > 1: (B, K, A), the standard deviation of the last call's candidates per element (normalised space), on the device"""
        return self.model.last_sample_spread

    @property
    def last_chunk_normalised(self) -> Optional[torch.Tensor]:
        """rtc: (B, K, A) copy of the chunks planned last, in normalised space (before the folded dataset statistics); None before the first plan.  (The core
        policy serves one environment and hands out its (K, A).)"""
        return self.model.last_chunk_normalised
