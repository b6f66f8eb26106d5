"""The step guard's state machine (csrc/optim_kernels.hip step_guard_decide_kernel / step_guard_observe_kernel; include/fastvla_hip.h fv_step_guard) restated
on the host: integers only, no float beyond isfinite.  `GuardRef.step(sumsq)` is one guarded step's decision and the state it leaves; `as_export()` is what
fv_step_guard_export must hand back after the same sequence.  Also the helpers the GPU tests build their gradient buffers with."""
import math

import torch


class GuardRef:
    def __init__(self, init_delta_log2=0, min_delta_log2=0, max_delta_log2=0, growth_interval=2000, backoff_log2=1, growth_log2=1, skip_on_saturation=True,
                 last_saturations=0):
        assert min_delta_log2 <= init_delta_log2 <= max_delta_log2 and growth_interval >= 1
        self.min, self.max, self.interval, self.backoff, self.growth, self.skip_sat = (int(min_delta_log2), int(max_delta_log2), int(growth_interval),
                                                                                        int(backoff_log2), int(growth_log2), bool(skip_on_saturation))
        self.delta_log2, self.good_steps = int(init_delta_log2), 0
        self.last_apply, self.last_inv_log2 = 1, -int(init_delta_log2)      # the exponent of the 1 / delta the last step used
        self.flag, self.last_saturations = 0, int(last_saturations)
        self.applied = self.skipped_nonfinite = self.skipped_saturated = self.saturated_applied = 0

    def observe(self, counter: int) -> None:
        """the saturation counter as a backward left it: a change sets the sticky flag"""
        if int(counter) != self.last_saturations:
            self.last_saturations = int(counter)
            self.flag = max(self.flag, 1)

    def set_flag(self, value=1) -> None:
        self.flag = int(value)

    def step(self, sumsq: float) -> bool:
        """one guarded step from the gradient's sum of squares -> applied?"""
        bad_nonfinite = not math.isfinite(sumsq)
        flagged = self.flag > 0
        bad_sat = self.skip_sat and flagged and self.delta_log2 > self.min
        self.last_apply, self.last_inv_log2 = int(not (bad_nonfinite or bad_sat)), -self.delta_log2
        if bad_nonfinite or bad_sat:
            if bad_nonfinite:
                self.skipped_nonfinite += 1
            else:
                self.skipped_saturated += 1
            self.delta_log2, self.good_steps = max(self.min, self.delta_log2 - self.backoff), 0
        else:
            self.applied += 1
            self.saturated_applied += int(flagged)
            self.good_steps += 1
            if self.good_steps >= self.interval:
                self.delta_log2, self.good_steps = min(self.max, self.delta_log2 + self.growth), 0
        self.flag = 0
        return bool(self.last_apply)

    def as_export(self) -> dict:
        return {"delta_log2": self.delta_log2, "good_steps": self.good_steps, "last_apply": self.last_apply, "last_inv_delta": math.ldexp(1.0, self.last_inv_log2),
                "flag": float(self.flag), "last_saturations": self.last_saturations, "applied": self.applied, "skipped_nonfinite": self.skipped_nonfinite,
                "skipped_saturated": self.skipped_saturated, "saturated_applied": self.saturated_applied}


def healthy_grads(n: int, seed: int) -> torch.Tensor:
    """n gradients of either sign with magnitudes in [1e-3, 10]: normal numbers whose products with a power of two 2^-24 .. 2^24 and whose squares stay normal,
    so that a power-of-two factor is exact all the way through the norm"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.empty(n).uniform_(math.log(1e-3), math.log(10.0), generator=g)).clamp_(1e-3, 10.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def step_buffers(n: int, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed + 1000)
    return dict(p=torch.randn(n, generator=g), g=healthy_grads(n, seed), m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.01,
                e=torch.randn(n, generator=g))
