"""The options of a policy beyond the reference's config -- action chunks, the loss and its weights, the flow head, its noise draws, solver, prefix
conditioning, samples, and real-time chunking -- resolved ONCE, before any engine exists: explicit argument, else the FASTVLA_* twin, else the default.
`resolve_policy_options` is the one entry point of both policy surfaces; `PolicyOptions` is what FastVLMWithExpert takes.  (The FastVLAPolicy docstring of
fastvla/modeling_fastvla.py has the semantics of every option.)"""
from __future__ import annotations

import inspect
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional


def pick(arg, env, cast, default, *, read: bool = True, error=None):
    """The explicit argument if given, else the environment twin `env` cast, else the default.  read=False: the twin is not read (twins that belong to a
    flow head pass action_head == "flow").  error(env, raw, cast) -> the message of the ValueError a twin the cast refuses gets; None lets the cast's own
    error escape."""
    if arg is not None:
        return arg
    raw = (os.environ.get(env) or "").strip() if read else ""
    if not raw:
        return default
    if error is None:
        return cast(raw)
    try:
        return cast(raw)
    except ValueError:
        raise ValueError(error(env, raw, cast)) from None


def parse_weight_list(raw: str, name: str, chunk: Optional[int] = None) -> List[float]:
    """"1,1,4" -> [1.0, 1.0, 4.0]; with `chunk` given also "discount:0.98" -> [0.98 ** k for k in range(chunk)].  ValueError for anything else."""
    raw = raw.strip()
    try:
        if chunk is not None and raw.lower().startswith("discount:"):
            gamma = float(raw.split(":", 1)[1])
            return [gamma ** k for k in range(int(chunk))]
        return [float(x) for x in raw.split(",") if x.strip()]
    except ValueError:
        raise ValueError(f"{name}: cannot read '{raw}' (a comma-separated list of numbers{', or discount:<gamma>' if chunk is not None else ''})") from None


def resolve_chunk_options(chunk_size=None, n_action_steps=None, action_loss=None, action_loss_beta=None, temporal_ensemble_coeff=None,
                          action_dim_weights=None, action_step_weights=None) -> Dict:
    """-> {"chunk_size", "n_action_steps", "loss", "beta", "temporal_ensemble_coeff", "dim_weights", "step_weights"}: explicit arguments, else the FASTVLA_*
    twins, else the defaults (1, 1, "mse", 1.0, None, None, None).  The last three also take False: off, whatever the twin says (what a checkpoint without
    a record of them asks for).  ValueError for n_action_steps outside 1 .. chunk_size, an unknown loss name, a non-positive beta, a non-finite coefficient,
    a coefficient together with n_action_steps != 1, or negative / non-finite weights (their lengths are checked against the head, in set_action_loss_weights)."""
    from fastvla_hip.engine import check_head_loss, check_loss_weights
    from fastvla_hip.ensemble import check_coeff

    K = pick(chunk_size, "FASTVLA_CHUNK_SIZE", int, 1)
    loss, beta, K = check_head_loss(pick(action_loss, "FASTVLA_ACTION_LOSS", str, "mse"), pick(action_loss_beta, "FASTVLA_ACTION_LOSS_BETA", float, 1.0), K)
    n = pick(n_action_steps, "FASTVLA_N_ACTION_STEPS", int, 1)
    if int(n) != n or n < 1 or n > K:
        raise ValueError(f"n_action_steps must be an integer in 1 .. chunk_size. Got n_action_steps={n}, chunk_size={K}.")
    coeff = pick(temporal_ensemble_coeff, "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", str, None)
    coeff = None if coeff is None or coeff is False else check_coeff(coeff)
    if coeff is not None and int(n) != 1:
        raise ValueError("n_action_steps must be 1 when using temporal ensembling: with it the policy is queried at every step. "
                         f"Got temporal_ensemble_coeff={coeff}, n_action_steps={n}.")
    dim_w = pick(action_dim_weights, "FASTVLA_ACTION_DIM_WEIGHTS", lambda r: parse_weight_list(r, "FASTVLA_ACTION_DIM_WEIGHTS"), None)
    step_w = pick(action_step_weights, "FASTVLA_ACTION_STEP_WEIGHTS", lambda r: parse_weight_list(r, "FASTVLA_ACTION_STEP_WEIGHTS", K), None)
    if isinstance(step_w, str):
        step_w = parse_weight_list(step_w, "action_step_weights", K)
    dim_w, step_w = (None if v is None or v is False else v for v in (dim_w, step_w))
    w = check_loss_weights(dim_w, step_w, len(dim_w) if dim_w is not None else 0, len(step_w) if step_w is not None else 0) or {"dim": None, "step": None}
    return {"chunk_size": K, "n_action_steps": int(n), "loss": loss, "beta": beta, "temporal_ensemble_coeff": coeff, "dim_weights": w["dim"],
            "step_weights": w["step"]}


FLOW_MIN_PERIOD, FLOW_MAX_PERIOD = 4e-3, 4.0      # pi0's periods of the time embedding
FLOW_DIST_A, FLOW_DIST_B = 0.0, 1.0                # logit-normal time: t = sigmoid(a + b n)


FLOW_TIME_PI0 = ("beta", 1.5, 1.0, (0.001, 1.0))   # pi0 / SmolVLA: tau ~ Beta(1.5, 1), t = 0.001 + 0.999 tau
FLOW_TIME_FORMS = "'uniform', 'logit_normal', 'beta:<alpha>,<beta>' (e.g. 'beta:1.5,1.0') or 'pi0' (= 'beta:1.5,1.0' on the range (0.001, 1.0))"


def parse_flow_time_dist(raw) -> Dict:
    """-> {"dist": "uniform" | "logit_normal" | "beta", "a", "b", "range": (lo, hi) or None, "name": the canonical string a checkpoint records}.  ValueError,
    giving the accepted forms, for anything else -- the bare word "beta" included: a Beta without its parameters names no distribution."""
    from fastvla_hip import _lib
    text = str(raw).strip().lower()
    if text in _lib.FLOW_TIME_DISTS:
        return {"dist": text, "a": FLOW_DIST_A, "b": FLOW_DIST_B, "range": None, "name": text}
    if text == "pi0":
        dist, a, b, rng = FLOW_TIME_PI0
        return {"dist": dist, "a": a, "b": b, "range": rng, "name": f"beta:{a!r},{b!r}"}
    if text.startswith("beta:"):
        try:
            a, b = (float(x) for x in text[5:].split(","))
        except ValueError:
            raise ValueError(f"flow_time_dist must be {FLOW_TIME_FORMS}, got {raw!r}") from None
        lo, hi = _lib.FLOW_BETA_RANGE
        if not (lo <= a <= hi and lo <= b <= hi):      # (NaN fails both)
            raise ValueError(f"flow_time_dist={raw!r}: both Beta parameters must lie in [{lo:g}, {hi:g}]")
        return {"dist": "beta", "a": a, "b": b, "range": None, "name": f"beta:{a!r},{b!r}"}
    raise ValueError(f"flow_time_dist must be {FLOW_TIME_FORMS}, got {raw!r}")


def parse_flow_time_range(raw, name: str = "flow_time_range"):
    """(lo, hi) or "lo:hi" -> (lo, hi) floats with 0 <= lo < hi <= 1; ValueError otherwise"""
    try:
        lo, hi = (float(x) for x in (raw.split(":") if isinstance(raw, str) else raw))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (lo, hi){' written lo:hi' if name.isupper() else ''} with 0 <= lo < hi <= 1, got {raw!r}") from None
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError(f"{name} must be (lo, hi) with 0 <= lo < hi <= 1, got {raw!r}")
    return lo, hi


def _flag(raw: str) -> bool:
    return raw.lower() not in ("0", "false", "no", "off")


BINS_DEFAULTS = {"bins": 256, "range": (-3.0, 3.0), "sigma": 0.0, "decode": "argmax"}


def parse_bins_range(raw, name: str = "FASTVLA_ACTION_BINS_RANGE"):
    """"lo:hi" -> (lo, hi) floats; ValueError for anything else (the order is check_head_bins' to refuse)"""
    try:
        lo, hi = (float(x) for x in str(raw).split(":"))
    except ValueError:
        raise ValueError(f"{name} must be written lo:hi, got {raw!r}") from None
    return lo, hi


def resolve_bins_options(action_bins=None, action_bins_range=None, action_bins_sigma=None, action_bins_decode=None, *, action_head: str, chunk_size: int = 1,
                         action_loss: str = "mse", action_dim: Optional[int] = None) -> Optional[Dict]:
    """-> FastVLAEngine.set_head_bins' keyword arguments {"bins", "range", "sigma", "decode"} for action_head == "bins", else None: explicit arguments, else the
    FASTVLA_ACTION_BINS / FASTVLA_ACTION_BINS_RANGE ("lo:hi") / FASTVLA_ACTION_BINS_SIGMA / FASTVLA_ACTION_BINS_DECODE twins -- read for a bins head only, like
    the FASTVLA_FLOW_* twins for flow --, else (256, (-3, 3), 0.0, "argmax").  ValueError, naming both settings and before any engine exists: an explicit
    action_bins_* with another head, an action_loss other than "mse", and check_head_bins' refusals (action_dim, when the caller has it, for the list length
    and the width limit)."""
    from fastvla_hip.engine import check_head_bins
    given = (("action_bins", action_bins), ("action_bins_range", action_bins_range), ("action_bins_sigma", action_bins_sigma), ("action_bins_decode", action_bins_decode))
    if action_head != "bins":
        for name, val in given:
            if val is not None:
                raise ValueError(f"{name} needs action_head='bins'. Got {name}={val!r}, action_head={action_head!r}.")
        return None
    if action_loss != "mse":
        raise ValueError(f"action_head='bins' trains with its own cross-entropy over the bins: action_loss must stay 'mse'. Got action_loss={action_loss!r}, action_head='bins'.")

    def twin(arg, env, cast, default):
        return pick(arg, env, cast, default, error=lambda env, raw, cast: f"{env} cannot be read: got {env}={raw!r} (action_head='bins')")

    bins = twin(action_bins, "FASTVLA_ACTION_BINS", int, BINS_DEFAULTS["bins"])
    rng = twin(action_bins_range, "FASTVLA_ACTION_BINS_RANGE", parse_bins_range, BINS_DEFAULTS["range"])
    if isinstance(rng, str):
        rng = parse_bins_range(rng, "action_bins_range")
    sigma = twin(action_bins_sigma, "FASTVLA_ACTION_BINS_SIGMA", float, BINS_DEFAULTS["sigma"])
    decode = twin(action_bins_decode, "FASTVLA_ACTION_BINS_DECODE", lambda r: r.lower(), BINS_DEFAULTS["decode"])
    return check_head_bins(bins, rng, sigma, decode, action_dim, chunk_size)


def resolve_flow_options(action_head=None, flow_steps=None, flow_time_dim=None, flow_time_dist=None, flow_time_range=None, flow_time_stratify=None, *,
                         flow_noise_draws: Optional[int] = None) -> Dict:
    """-> {"action_head": "regression" | "flow", "steps", "flow": FastVLAEngine.set_head_flow's keyword arguments or None}: explicit arguments, else the
    FASTVLA_ACTION_HEAD / FASTVLA_FLOW_STEPS / FASTVLA_FLOW_TIME_DIM / FASTVLA_FLOW_TIME_DIST twins, else ("regression", 10, 64, "uniform").  A regression head
    neither reads nor checks the flow twins.  ValueError for an
    unknown head or time distribution, steps < 1, a time_dim that is not a positive even integer.
    The training time beyond set_head_flow's two distributions -- flow_time_dist "beta:<alpha>,<beta>" | "pi0", flow_time_range=(lo, hi)
    (FASTVLA_FLOW_TIME_RANGE="lo:hi"), flow_time_stratify (FASTVLA_FLOW_TIME_STRATIFY) -- adds ONE key, and only when asked for:
    "time": FastVLAEngine.set_head_flow_time's keyword arguments plus "name", the string a checkpoint records.  flow_time_range / flow_time_stratify = False:
    off, whatever the twin says.  flow_noise_draws: the resolved S, when the caller has it -- ValueError, naming both settings, for strata with one draw;
    and for any of the three given explicitly with a regression head."""
    from fastvla_hip import _lib

    head = str(pick(action_head, "FASTVLA_ACTION_HEAD", str, "regression")).lower()
    if head not in ("regression", "flow", "bins"):
        raise ValueError(f"action_head must be 'regression', 'flow' or 'bins', got {head!r}")
    if head != "flow":      # the FASTVLA_FLOW_* twins are read and checked for a flow head only: a stray value cannot make a regression policy (or its load) raise
        for name, val in (("flow_time_dist", flow_time_dist), ("flow_time_range", flow_time_range), ("flow_time_stratify", flow_time_stratify)):
            if val is not None and val is not False:
                raise ValueError(f"{name} needs action_head='flow' (the {head} head draws no time). Got {name}={val!r}, action_head={head!r}.")
        if head == "bins" and (flow_steps is not None or flow_time_dim is not None):
            name, val = ("flow_steps", flow_steps) if flow_steps is not None else ("flow_time_dim", flow_time_dim)
            raise ValueError(f"{name} needs action_head='flow' (the bins head integrates nothing). Got {name}={val!r}, action_head={head!r}.")
        return {"action_head": head, "steps": 10, "flow": None}
    steps, dim = pick(flow_steps, "FASTVLA_FLOW_STEPS", int, 10), pick(flow_time_dim, "FASTVLA_FLOW_TIME_DIM", int, 64)
    tdist = parse_flow_time_dist(pick(flow_time_dist, "FASTVLA_FLOW_TIME_DIST", str, "uniform"))
    dist = tdist["dist"] if tdist["dist"] in _lib.FLOW_TIME_DISTS else "uniform"      # (set_head_flow's own: a Beta rides on the uniform head)
    if int(steps) != steps or steps < 1:
        raise ValueError(f"flow_steps must be an integer >= 1, got {steps}")
    if int(dim) != dim or dim < 2 or dim % 2:
        raise ValueError(f"flow_time_dim must be a positive even integer, got {dim}")
    flow = dict(time_dim=int(dim), min_period=FLOW_MIN_PERIOD, max_period=FLOW_MAX_PERIOD, time_dist=dist, dist_a=FLOW_DIST_A, dist_b=FLOW_DIST_B)
    out = {"action_head": head, "steps": int(steps), "flow": flow}
    rng = None if flow_time_range is False else pick(flow_time_range, "FASTVLA_FLOW_TIME_RANGE", lambda r: parse_flow_time_range(r, "FASTVLA_FLOW_TIME_RANGE"), None)
    rng = tdist["range"] if rng is None else parse_flow_time_range(rng)      # (an explicit range wins over pi0's)
    strat = False if flow_time_stratify is False else pick(flow_time_stratify, "FASTVLA_FLOW_TIME_STRATIFY", _flag, False)
    if not isinstance(strat, (bool, int)) or strat not in (0, 1):
        raise ValueError(f"flow_time_stratify must be a bool, got {strat!r}")
    if tdist["dist"] == "beta" or rng is not None or strat:
        lo, hi = rng or (0.0, 1.0)
        out["time"] = dict(dist=tdist["dist"], a=float(tdist["a"]), b=float(tdist["b"]), t_lo=float(lo), t_hi=float(hi), stratify=bool(strat), name=tdist["name"])
    if flow_noise_draws is not None:
        check_flow_time_draws(out.get("time"), flow_noise_draws)
    return out


def check_flow_time_draws(time: Optional[Dict], draws: int) -> None:
    """strata are dealt to the draws of one observation: ValueError, naming both settings, for flow_time_stratify with one draw"""
    if time is not None and time["stratify"] and int(draws) == 1:
        raise ValueError("flow_time_stratify=True needs flow_noise_draws > 1: the strata are dealt to the draws of one observation. "
                         f"Got flow_time_stratify=True, flow_noise_draws={draws}.")


def resolve_flow_solver(flow_solver=None, *, action_head: str) -> str:
    """-> "euler" | "midpoint" | "heun" | "rk4", the integrator of a flow head's samplers: the explicit argument, else FASTVLA_FLOW_SOLVER, else "euler".  The
    twin is read and checked for a flow head only, like the other FASTVLA_FLOW_* twins.  ValueError, naming both settings and before any engine exists, for
    an unknown name or an explicit flow_solver with the regression head."""
    from fastvla_hip.engine import check_flow_solver
    if flow_solver is not None:      # an explicit argument is checked whatever the head is
        try:
            name = check_flow_solver(flow_solver)
        except ValueError:
            raise ValueError(f"flow_solver must be 'euler', 'midpoint', 'heun' or 'rk4'. Got flow_solver={flow_solver!r}, action_head={action_head!r}.") from None
        if action_head != "flow":
            raise ValueError(f"flow_solver needs action_head='flow' (the regression head integrates nothing). Got flow_solver={name!r}, action_head={action_head!r}.")
        return name
    return pick(None, "FASTVLA_FLOW_SOLVER", check_flow_solver, "euler", read=action_head == "flow", error=lambda env, raw, cast: (
        f"FASTVLA_FLOW_SOLVER must be 'euler', 'midpoint', 'heun' or 'rk4'. Got FASTVLA_FLOW_SOLVER={raw!r}, action_head={action_head!r}."))


def resolve_flow_samples(flow_samples=None, flow_select=None, flow_coherence_decay=None, *, action_head: str, chunk_size: int, rtc_method: Optional[str] = None) -> Dict:
    """-> {"samples", "select", "decay"}: several samples per observation at inference (fastvla_hip/select.py).  Explicit arguments, else the FASTVLA_FLOW_SAMPLES /
    FASTVLA_FLOW_SELECT / FASTVLA_FLOW_COHERENCE_DECAY twins -- read for a flow head only --, else (1, None, 0.5).  ValueError naming both settings, before any
    engine exists: a regression head, samples outside 1 .. 16, a select name with one sample, "coherent" with chunk_size = 1, rtc_method="guidance" with
    several samples."""
    from fastvla_hip.select import check_flow_select, coherence_weights
    flow = action_head == "flow"

    def twin(arg, env, cast):
        return pick(arg, env, cast, None, read=flow, error=lambda env, raw, cast: (
            f"{env} must be {'an integer' if cast is int else 'a number'}, got {env}={raw!r} (action_head={action_head!r})"))

    samples = twin(flow_samples, "FASTVLA_FLOW_SAMPLES", int)
    select = twin(flow_select, "FASTVLA_FLOW_SELECT", lambda r: r.lower())
    decay = twin(flow_coherence_decay, "FASTVLA_FLOW_COHERENCE_DECAY", float)
    if decay is not None and not flow:
        raise ValueError(f"flow_coherence_decay={decay!r} / flow_samples={samples!r} need action_head='flow', got action_head={action_head!r}")
    samples, select = check_flow_select(samples, select, action_head=action_head, chunk_size=chunk_size, rtc_method=rtc_method)
    decay = 0.5 if decay is None else decay
    coherence_weights(max(int(chunk_size), 1), decay)      # (checks the decay)
    return {"samples": samples, "select": select, "decay": float(decay)}


def resolve_flow_noise_draws(flow_noise_draws=None, *, action_head: str) -> int:
    """-> S, the noise draws per observation of a flow head's training and loss evaluations: the explicit argument, else FASTVLA_FLOW_NOISE_DRAWS, else 1.  The
    twin is read and checked for a flow head only, like the other FASTVLA_FLOW_* twins.  ValueError, naming both settings and before any engine exists, for
    an explicit S > 1 with the regression head, a non-integer, or a value outside 1 .. 16."""
    from fastvla_hip.engine import check_flow_draws
    if flow_noise_draws is not None:      # an explicit argument is checked whatever the head is
        try:
            draws = check_flow_draws(flow_noise_draws)
        except ValueError:
            raise ValueError(f"flow_noise_draws must be an integer 1 .. 16. Got flow_noise_draws={flow_noise_draws!r}, action_head={action_head!r}.") from None
        if draws > 1 and action_head != "flow":
            raise ValueError("flow_noise_draws > 1 needs action_head='flow' (the regression head draws no noise). "
                             f"Got flow_noise_draws={draws}, action_head={action_head!r}.")
        return draws
    return pick(None, "FASTVLA_FLOW_NOISE_DRAWS", lambda r: check_flow_draws(int(r)), 1, read=action_head == "flow", error=lambda env, raw, cast: (
        f"FASTVLA_FLOW_NOISE_DRAWS must be an integer 1 .. 16. Got FASTVLA_FLOW_NOISE_DRAWS={raw!r}, action_head={action_head!r}."))


def resolve_prefix_options(flow_prefix_max_delay=None, flow_prefix_delay_dist=None, flow_prefix_delay_rate=None, *, action_head: str, chunk_size: int,
                           temporal_ensemble_coeff=None) -> Optional[Dict]:
    """-> fastvla_hip.prefix.check_prefix_config's record {"chunk", "max_delay", "dist", "rate", "thresholds"} or None (off): explicit arguments, else the
    FASTVLA_FLOW_PREFIX_MAX_DELAY / _DELAY_DIST / _DELAY_RATE twins (read for a flow head only, like the other FASTVLA_FLOW_* twins), else off.
    flow_prefix_max_delay=False: off whatever the twin says.  ValueError, naming both settings and before any engine exists, for a regression head,
    chunk_size == 1, a delay that does not fit the chunk, or temporal_ensemble_coeff."""
    from fastvla_hip import prefix as _prefix

    def twin(arg, env, cast, default):
        return pick(arg, env, cast, default, error=lambda env, raw, cast: f"{env} must be {cast.__name__}, got {raw!r}")

    D = flow_prefix_max_delay
    if D is False:
        return None
    if D is None:
        if action_head != "flow":
            return None
        D = twin(None, "FASTVLA_FLOW_PREFIX_MAX_DELAY", int, None)
        if D is None or D == 0:
            return None
    dist = str(twin(flow_prefix_delay_dist, "FASTVLA_FLOW_PREFIX_DELAY_DIST", str, "uniform")).lower()
    rate = twin(flow_prefix_delay_rate, "FASTVLA_FLOW_PREFIX_DELAY_RATE", float, 0.5)
    return _prefix.check_prefix_config(D, action_head=action_head, chunk_size=chunk_size, temporal_ensemble_coeff=temporal_ensemble_coeff, dist=dist, rate=rate)


def resolve_rtc_options(rtc=None, rtc_schedule=None, rtc_max_guidance_weight=None, rtc_execution_horizon=None, *, action_head: str, chunk_size: int,
                        n_action_steps: int, temporal_ensemble_coeff=None, rtc_method=None, rtc_prefix_steps=None, prefix: Optional[Dict] = None) -> Optional[Dict]:
    """-> {"schedule", "max_guidance_weight", "execution_horizon"} or None (off): explicit arguments, else the FASTVLA_RTC / FASTVLA_RTC_SCHEDULE /
    FASTVLA_RTC_MAX_GUIDANCE_WEIGHT / FASTVLA_RTC_EXECUTION_HORIZON twins, else (off, "exp", 5.0, n_action_steps).  The other twins are read and checked
    only when real-time chunking is on.  ValueError, naming both settings, for rtc with a regression head, with chunk_size == 1, with
    temporal_ensemble_coeff, or with an execution horizon that does not fit the chunk; for an unknown schedule or a non-positive / non-finite weight."""
    import math
    from fastvla_hip.rtc import check_rtc

    on = pick(rtc, "FASTVLA_RTC", lambda r: r.lower() not in ("0", "false", "no", "off"), False)
    if not on:
        return None
    if action_head != "flow":
        raise ValueError(f"rtc=True needs action_head='flow' (guidance is defined for the flow sampler only). Got rtc={on}, action_head={action_head!r}.")
    if chunk_size == 1:
        raise ValueError(f"rtc=True needs chunk_size > 1: there is no overlap between chunks of one step. Got rtc={on}, chunk_size={chunk_size}.")
    if temporal_ensemble_coeff is not None:
        raise ValueError("rtc and temporal_ensemble_coeff cannot be combined: one joins chunks by guidance, the other by averaging them. "
                         f"Got rtc={on}, temporal_ensemble_coeff={temporal_ensemble_coeff}.")
    # rtc_method (FASTVLA_RTC_METHOD): "guidance" (the default: everything below, on either head width) or "prefix" -- the prefix sampler of a head trained
    # with flow_prefix_max_delay = D: a re-plan PINS its first min(rtc_prefix_steps, D, K - shift) steps to the previous chunk; no guidance, no schedule, no beta
    method = str(pick(rtc_method, "FASTVLA_RTC_METHOD", str, "guidance")).lower()
    if method not in ("guidance", "prefix"):
        raise ValueError(f"rtc_method must be 'guidance' or 'prefix', got {method!r}")
    if method == "prefix":
        if prefix is None:
            raise ValueError("rtc_method='prefix' needs a head trained with action-prefix conditioning. Got rtc_method='prefix', flow_prefix_max_delay=None.")
        for name, val in (("rtc_schedule", rtc_schedule), ("rtc_max_guidance_weight", rtc_max_guidance_weight), ("rtc_execution_horizon", rtc_execution_horizon)):
            if val is not None:
                raise ValueError(f"{name} belongs to rtc_method='guidance': the prefix sampler has no guidance to shape. Got {name}={val!r}, rtc_method='prefix'.")
        D = int(prefix["max_delay"])
        steps = pick(rtc_prefix_steps, "FASTVLA_RTC_PREFIX_STEPS", int, D)
        if isinstance(steps, bool) or not isinstance(steps, int) or not 0 <= steps <= D:
            raise ValueError(f"rtc_prefix_steps must be an integer in 0 .. flow_prefix_max_delay. Got rtc_prefix_steps={steps!r}, flow_prefix_max_delay={D}.")
        return {"method": "prefix", "prefix_steps": int(steps), "max_delay": D}
    if rtc_prefix_steps is not None:
        raise ValueError(f"rtc_prefix_steps needs rtc_method='prefix'. Got rtc_prefix_steps={rtc_prefix_steps!r}, rtc_method={method!r}.")
    schedule = str(pick(rtc_schedule, "FASTVLA_RTC_SCHEDULE", str, "exp")).lower()
    beta = pick(rtc_max_guidance_weight, "FASTVLA_RTC_MAX_GUIDANCE_WEIGHT", float, 5.0)
    s = pick(rtc_execution_horizon, "FASTVLA_RTC_EXECUTION_HORIZON", int, n_action_steps)
    try:
        beta = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"rtc_max_guidance_weight must be a finite number > 0, got {beta!r}") from None
    if not math.isfinite(beta) or beta <= 0.0:
        raise ValueError(f"rtc_max_guidance_weight must be a finite number > 0, got {beta!r}")
    if isinstance(s, int) and not isinstance(s, bool) and s > chunk_size:
        raise ValueError(f"rtc_execution_horizon must not exceed chunk_size (inference_delay + execution_horizon <= chunk_size). "
                         f"Got rtc_execution_horizon={s}, chunk_size={chunk_size}.")
    check_rtc(chunk_size, 0, s, schedule)
    return {"schedule": schedule, "max_guidance_weight": beta, "execution_horizon": int(s)}


@dataclass(frozen=True)
class PolicyOptions:
    """What resolve_policy_options resolved; the defaults are a policy that asked for nothing (the reference's FastVLMWithExpert(config))."""
    chunk: Dict = field(default_factory=lambda: {"chunk_size": 1, "n_action_steps": 1, "loss": "mse", "beta": 1.0, "temporal_ensemble_coeff": None,
                                                 "dim_weights": None, "step_weights": None})      # resolve_chunk_options' record
    action_head: str = "regression"
    flow: Optional[Dict] = None      # FastVLAEngine.set_head_flow's keyword arguments, None = the regression head
    flow_time: Optional[Dict] = None      # resolve_flow_options' "time": set_head_flow_time's keyword arguments + "name"; None = set_head_flow's own distribution
    flow_steps: int = 10
    flow_seed: Optional[int] = None      # None: torch's initial seed
    noise_draws: int = 1
    solver: str = "euler"
    prefix: Optional[Dict] = None      # fastvla_hip.prefix.check_prefix_config's record
    rtc: Optional[Dict] = None      # resolve_rtc_options' record
    samples: int = 1
    select: Optional[str] = None
    decay: float = 0.5
    bins: Optional[Dict] = None      # resolve_bins_options' record (set_head_bins' keyword arguments), None = no binned head


def resolve_policy_options(*, chunk_size=None, n_action_steps=None, action_loss=None, action_loss_beta=None, temporal_ensemble_coeff=None,
                           action_dim_weights=None, action_step_weights=None, action_head=None, flow_steps=None, flow_time_dim=None, flow_time_dist=None,
                           flow_time_range=None, flow_time_stratify=None, flow_seed=None, rtc=None, rtc_schedule=None, rtc_max_guidance_weight=None, rtc_execution_horizon=None, flow_noise_draws=None,
                           flow_prefix_max_delay=None, flow_prefix_delay_dist=None, flow_prefix_delay_rate=None, rtc_method=None, rtc_prefix_steps=None,
                           flow_solver=None, flow_samples=None, flow_select=None, flow_coherence_decay=None, action_bins=None, action_bins_range=None,
                           action_bins_sigma=None, action_bins_decode=None, action_dim: Optional[int] = None) -> PolicyOptions:
    """Every option of a policy constructor, resolved and refused before any engine exists.  The resolvers run in this order -- chunk, flow, noise draws,
    solver, prefix, rtc, samples, bins -- and the first ValueError wins.  action_dim: the config's A, when the caller has it (the bins head's width limit and
    per-dimension ranges are checked against it here; HeadSpec checks them again).  A bins head refuses every flow_* / rtc* option by the resolvers' own
    "needs action_head='flow'" refusals."""
    chunk = resolve_chunk_options(chunk_size, n_action_steps, action_loss, action_loss_beta, temporal_ensemble_coeff, action_dim_weights, action_step_weights)
    K, coeff = chunk["chunk_size"], chunk["temporal_ensemble_coeff"]
    fopts = resolve_flow_options(action_head, flow_steps, flow_time_dim, flow_time_dist, flow_time_range, flow_time_stratify)
    head = fopts["action_head"]
    draws = resolve_flow_noise_draws(flow_noise_draws, action_head=head)
    check_flow_time_draws(fopts.get("time"), draws)
    solver = resolve_flow_solver(flow_solver, action_head=head)
    prefix = resolve_prefix_options(flow_prefix_max_delay, flow_prefix_delay_dist, flow_prefix_delay_rate, action_head=head, chunk_size=K,
                                    temporal_ensemble_coeff=coeff)
    ropts = resolve_rtc_options(rtc, rtc_schedule, rtc_max_guidance_weight, rtc_execution_horizon, action_head=head, chunk_size=K,
                                n_action_steps=chunk["n_action_steps"], temporal_ensemble_coeff=coeff, rtc_method=rtc_method, rtc_prefix_steps=rtc_prefix_steps,
                                prefix=prefix)
    sopts = resolve_flow_samples(flow_samples, flow_select, flow_coherence_decay, action_head=head, chunk_size=K,
                                 rtc_method=None if ropts is None else ropts.get("method", "guidance"))
    if head == "bins":      # the options whose resolvers let an explicit value pass for a head that is not flow
        for name, val in (("flow_seed", flow_seed), ("flow_noise_draws", flow_noise_draws), ("flow_prefix_max_delay", flow_prefix_max_delay), ("flow_select", flow_select),
                          ("flow_samples", flow_samples), ("rtc_method", rtc_method), ("rtc_schedule", rtc_schedule), ("rtc_max_guidance_weight", rtc_max_guidance_weight),
                          ("rtc_execution_horizon", rtc_execution_horizon), ("rtc_prefix_steps", rtc_prefix_steps), ("flow_prefix_delay_dist", flow_prefix_delay_dist),
                          ("flow_prefix_delay_rate", flow_prefix_delay_rate), ("rtc", rtc)):
            if val is not None and val is not False:
                raise ValueError(f"{name} needs action_head='flow' (the bins head samples nothing). Got {name}={val!r}, action_head='bins'.")
    bins = resolve_bins_options(action_bins, action_bins_range, action_bins_sigma, action_bins_decode, action_head=head, chunk_size=K, action_loss=chunk["loss"],
                                action_dim=action_dim)
    return PolicyOptions(bins=bins, chunk=chunk, action_head=head, flow=fopts["flow"], flow_time=fopts.get("time"), flow_steps=fopts["steps"], flow_seed=flow_seed, noise_draws=draws, solver=solver,
                         prefix=prefix, rtc=ropts, samples=sopts["samples"], select=sopts["select"], decay=sopts["decay"])


POLICY_KEYWORDS = frozenset(inspect.signature(resolve_policy_options).parameters)      # (a surface that takes **kwargs passes these on and ignores the rest)
