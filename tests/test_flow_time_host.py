"""CPU: the float64 reference of the flow head's training-time distributions (tests/flow_time_util.py) held to facts of its own -- closed forms, the symmetry
and the round trip of the inverse incomplete beta function, the strata --, the reference of the loss by time bucket, and the host side of the options:
resolution, twins, every refusal, HeadSpec, the checkpoint record on both surfaces."""
import numpy as np
import pytest
from scipy import special

import flow_time_util as tu
import flow_util as fu

TIME_ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_STEPS", "FASTVLA_FLOW_TIME_DIM", "FASTVLA_FLOW_TIME_DIST", "FASTVLA_FLOW_TIME_RANGE", "FASTVLA_FLOW_TIME_STRATIFY",
            "FASTVLA_FLOW_SOLVER", "FASTVLA_RTC", "FASTVLA_FLOW_PREFIX_MAX_DELAY", "FASTVLA_FLOW_NOISE_DRAWS", "FASTVLA_FLOW_SAMPLES")


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_inverse_beta_against_closed_forms():
    """scipy's betaincinv at the edge integers, every stratum of S = 1, 3, 16: the identity, u^(1/a), 1 - (1 - u)^(1/b), sin^2(pi u / 2) and the symmetry.
    Each closed form is itself a few float64 roundings of the true value; 1e-14 relative to max(tau, 2^-24) is a thousand times inside the GPU tests' bar"""
    k = np.array(tu.EDGE_K, np.float64)
    worst = worst_sym = 0.0
    for S in (1, 3, 16):
        for s in range(S):
            u = tu.uniform_u(k, s, S, stratify=True)
            scale = lambda ref: np.maximum(np.abs(ref), tu.U24)  # noqa: E731
            assert np.array_equal(tu.tau_ref("beta", 1.0, 1.0, u), u)
            for a in (0.25, 1.5, 8.0):
                ref = u ** (1.0 / a)
                worst = max(worst, float((np.abs(tu.tau_ref("beta", a, 1.0, u) - ref) / scale(ref)).max()))
            for b in (0.25, 0.75, 5.0):
                ref = -np.expm1(np.log1p(-u) / b)
                worst = max(worst, float((np.abs(tu.tau_ref("beta", 1.0, b, u) - ref) / scale(ref)).max()))
            ref = np.sin(np.pi * u / 2.0) ** 2
            worst = max(worst, float((np.abs(tu.tau_ref("beta", 0.5, 0.5, u) - ref) / scale(ref)).max()))
            # the symmetry where 1 - u is exact in float64; the subtraction 1 - tau' rounds at 2^-53, so the identity is an ABSOLUTE statement
            exact = (1.0 - (1.0 - u)) == u
            for a, b in tu.BETAS:
                x, y = tu.tau_ref("beta", a, b, u[exact]), 1.0 - tu.tau_ref("beta", b, a, 1.0 - u[exact])
                worst_sym = max(worst_sym, float(np.abs(x - y).max()))
    print(f"[flow time host] closed forms: worst error / max(tau, 2^-24) = {worst:.2e}; symmetry: worst absolute difference {worst_sym:.2e}")
    assert worst <= 1e-14 and worst_sym <= 1e-15


def test_reference_inverse_beta_round_trips():
    """I_{I^-1_u}(a, b) = u, turned into an error of tau through the density: |I(tau) - u| / pdf(tau) <= 1e-12 max(tau, 2^-24) (measured: 4e-14), for every (a, b) of the GPU
    tests and the corners of the accepted range"""
    k = np.array(tu.EDGE_K[1:], np.float64)
    worst = 0.0
    for a, b in tu.BETAS + ((0.25, 0.25), (32.0, 32.0), (32.0, 0.25), (0.25, 32.0)):
        for S in (1, 3, 16):
            for s in range(S):
                u = tu.uniform_u(k, s, S, stratify=True)
                tau = tu.tau_ref("beta", a, b, u)
                assert bool((np.diff(tau) >= 0).all()) and bool((tau >= 0).all()) and bool((tau <= 1).all())
                inner = (tau > 0) & (tau < 1)
                with np.errstate(over="ignore"):
                    pdf = np.exp((a - 1) * np.log(tau[inner]) + (b - 1) * np.log1p(-tau[inner]) - special.betaln(a, b))
                t, uu = tau[inner], u[inner]      # (the residual in the tail the point lies in: I_tau(a, b) near 1 has lost the bits of 1 - u)
                res = np.where(uu <= 0.5, special.betainc(a, b, t) - uu, (1.0 - uu) - special.betainc(b, a, 1.0 - t))
                err = np.abs(res) / pdf / np.maximum(t, tu.U24)
                worst = max(worst, float(err.max()))
    print(f"[flow time host] round trip: worst error of tau / max(tau, 2^-24) = {worst:.2e}")
    assert worst <= 1e-12


def test_strata_and_the_logit_normal_reference():
    # the float64 u of draw s lies in stratum s, at both ends of the integer's range
    for S in (2, 3, 16):
        for s in range(S):
            for k in (0, 2 ** 24 - 1):
                u = float(tu.uniform_u(k, s, S, stratify=True))
                assert s / S <= u < (s + 1) / S, (S, s, k, u)
    assert np.array_equal(tu.uniform_u(np.arange(5), 2, 3, stratify=False), np.arange(5) * tu.U24)      # no strata without the switch ...
    assert np.array_equal(tu.uniform_u(np.arange(5), 0, 1, stratify=True), np.arange(5) * tu.U24)       # ... nor with one draw
    # logit-normal through the inverse normal CDF: u = 0 gives 0, the median is sigmoid(a), monotone in u
    u = tu.uniform_u(np.array(tu.EDGE_K), 1, 3, stratify=True)
    tau = tu.tau_ref("logit_normal", 0.3, 1.7, np.concatenate([[0.0, 0.5], u]))
    assert tau[0] == 0.0 and abs(tau[1] - 1.0 / (1.0 + np.exp(-float(np.float32(0.3))))) <= 1e-16 and bool((np.diff(tau[2:]) > 0).all())
    # the range uses the fp32 values the spec carries
    assert float(tu.scale_ref(0.0, 0.001, 1.0)) == float(np.float32(0.001)) and float(tu.scale_ref(1.0, 0.001, 1.0)) == 1.0
    # draw_t_ref: Beta(1, 1) on (0, 1) is the uniform draw, draw-major over the offsets o + (s << 56)
    t = tu.draw_t_ref(9, 3, 77, 5, "beta", 1.0, 1.0)
    for s in range(3):
        assert np.array_equal(t[s * 9:(s + 1) * 9].astype(np.float32), fu.draw_t_uniform(9, 77, 5 + (s << 56)))
    # the bar: one fp32 ulp at max(t, 2^-24)
    assert float(tu.time_bar(0.0)) == 2.0 ** -47 and float(tu.time_bar(0.75)) == 2.0 ** -24 and float(tu.time_bar(1e-30)) == 2.0 ** -47


def test_loss_per_time_reference():
    rng = np.random.default_rng(0)
    R, B, K, A = 6, 3, 2, 2
    v, u = rng.standard_normal((R, K * A)), rng.standard_normal((R, K * A))
    t = np.array([0.0, 0.0999, 0.1, 0.95, 1.0, 1.5], np.float32)
    assert list(tu.bucket_of(t, 10)) == [0, 0, 1, 9, 9, 9] and list(tu.bucket_of(t, 1)) == [0] * 6      # t = 1.0 lands in the last bucket; beyond it is clamped
    pad = np.zeros((B, K), bool)
    pad[1, 1] = True
    sums, counts = tu.loss_per_time_ref(v, u, t, 10, pad, B, K)
    assert list(counts) == [6, 4, 0, 0, 0, 0, 0, 0, 0, 10] and sums[2] == 0.0      # rows 1 and 4 are observation 1: two elements each are padded
    d = (v - u) ** 2
    assert abs(sums[0] - (d[0].sum() + d[1, :2].sum())) <= 1e-15 and abs(sums.sum() - (d.sum() - d[1, 2:].sum() - d[4, 2:].sum())) <= 1e-14


# ------------------------------------------------------------------------------------------------------------------ the options
def test_time_options_resolve_and_refuse(monkeypatch):
    from fastvla_hip import _lib
    from vla_fastvlm.fastvla.options import resolve_flow_options, resolve_policy_options
    for k in TIME_ENV:
        monkeypatch.delenv(k, raising=False)
    want = dict(time_dim=64, min_period=4e-3, max_period=4.0, time_dist="uniform", dist_a=0.0, dist_b=1.0)
    # today's arguments give today's dictionaries, with no new key
    assert resolve_flow_options() == {"action_head": "regression", "steps": 10, "flow": None}
    assert resolve_flow_options("flow") == {"action_head": "flow", "steps": 10, "flow": want}
    assert resolve_flow_options("flow", flow_time_dist="logit_normal") == {"action_head": "flow", "steps": 10, "flow": {**want, "time_dist": "logit_normal"}}
    assert _lib.FLOW_TIME_DISTS == {"uniform": 0, "logit_normal": 1} and resolve_policy_options(action_head="flow").flow_time is None
    # the new settings appear under a key of their own
    pi0 = dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0, stratify=False, name="beta:1.5,1.0")
    assert resolve_flow_options("flow", flow_time_dist="pi0") == {"action_head": "flow", "steps": 10, "flow": want, "time": pi0}
    assert resolve_flow_options("flow", flow_time_dist="beta:1.5,1.0")["time"] == {**pi0, "t_lo": 0.0}
    assert resolve_flow_options("flow", flow_time_dist="Beta:2, 5")["time"] == dict(dist="beta", a=2.0, b=5.0, t_lo=0.0, t_hi=1.0, stratify=False, name="beta:2.0,5.0")
    assert resolve_flow_options("flow", flow_time_dist="pi0", flow_time_range=(0.0, 0.5))["time"] == {**pi0, "t_lo": 0.0, "t_hi": 0.5}      # an explicit range wins
    r = resolve_flow_options("flow", flow_time_dist="logit_normal", flow_time_range=(0.1, 0.9))
    assert r["flow"]["time_dist"] == "logit_normal" and r["time"] == dict(dist="logit_normal", a=0.0, b=1.0, t_lo=0.1, t_hi=0.9, stratify=False, name="logit_normal")
    o = resolve_policy_options(action_head="flow", flow_time_stratify=True, flow_noise_draws=3)
    assert o.flow == want and o.flow_time == dict(dist="uniform", a=0.0, b=1.0, t_lo=0.0, t_hi=1.0, stratify=True, name="uniform") and o.noise_draws == 3
    # the twins take the same strings, for a flow head only; the argument beats them; False switches range and strata off whatever the twin says
    monkeypatch.setenv("FASTVLA_FLOW_TIME_DIST", "pi0")
    monkeypatch.setenv("FASTVLA_FLOW_TIME_RANGE", "0.25:0.75")
    monkeypatch.setenv("FASTVLA_FLOW_TIME_STRATIFY", "1")
    assert resolve_flow_options() == {"action_head": "regression", "steps": 10, "flow": None}
    assert resolve_flow_options("flow")["time"] == {**pi0, "t_lo": 0.25, "t_hi": 0.75, "stratify": True}
    assert resolve_flow_options("flow", flow_time_dist="uniform", flow_time_range=False, flow_time_stratify=False) == {"action_head": "flow", "steps": 10, "flow": want}
    with pytest.raises(ValueError, match="flow_time_stratify.*flow_noise_draws"):
        resolve_policy_options(action_head="flow")                                       # the twin's strata with one draw
    assert resolve_policy_options(action_head="flow", flow_noise_draws=2).flow_time["stratify"] is True
    monkeypatch.setenv("FASTVLA_FLOW_TIME_RANGE", "0.5")
    with pytest.raises(ValueError, match="FASTVLA_FLOW_TIME_RANGE"):
        resolve_flow_options("flow")
    for k in TIME_ENV:
        monkeypatch.delenv(k, raising=False)
    # every refusal, before any engine exists
    with pytest.raises(ValueError, match="beta:<alpha>,<beta>"):                          # the bare word: the message gives the accepted form
        resolve_flow_options("flow", flow_time_dist="beta")
    for bad in ("beta:", "beta:1.5", "beta:1,2,3", "beta:a,b", "beta:0.2,1", "beta:1,33", "beta:nan,1", "gamma:1,1", ""):
        with pytest.raises(ValueError, match="flow_time_dist"):
            resolve_flow_options("flow", flow_time_dist=bad)
    for bad in ((0.5, 0.5), (0.6, 0.4), (-0.1, 1.0), (0.0, 1.1), (0.0, float("nan")), (0.0,), "0:1:2", 3):
        with pytest.raises(ValueError, match="flow_time_range"):
            resolve_flow_options("flow", flow_time_range=bad)
    with pytest.raises(ValueError, match="flow_time_stratify"):
        resolve_flow_options("flow", flow_time_stratify="yes")
    with pytest.raises(ValueError, match="flow_time_stratify.*flow_noise_draws"):
        resolve_policy_options(action_head="flow", flow_time_stratify=True, flow_noise_draws=1)
    with pytest.raises(ValueError, match="flow_time_stratify.*flow_noise_draws"):
        resolve_flow_options("flow", flow_time_stratify=True, flow_noise_draws=1)
    for kw in (dict(flow_time_dist="pi0"), dict(flow_time_dist="uniform"), dict(flow_time_range=(0.0, 1.0)), dict(flow_time_stratify=True)):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=f"{name}.*regression"):
            resolve_policy_options(action_head="regression", **kw)
        with pytest.raises(ValueError, match=f"{name}.*regression"):
            resolve_policy_options(**kw)                                                   # (the default head is the regression head)


def test_engine_checks_and_head_spec():
    from fastvla_hip.engine import check_flow_time
    from fastvla_hip.head_spec import HeadSpec
    assert check_flow_time("Beta", 1.5, 1, 0.001, 1, False) == dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0, stratify=False)
    assert check_flow_time("logit_normal", -3.0, 100.0, 0, 1, 1)["stratify"] is True      # (a logit-normal's a and b are any finite numbers)
    for bad in (("gamma", 1, 1, 0, 1, 0), ("beta", 0.2, 1, 0, 1, 0), ("beta", 1, 32.5, 0, 1, 0), ("uniform", float("inf"), 1, 0, 1, 0), ("uniform", 0, 1, 0.5, 0.5, 0),
                ("uniform", 0, 1, 0, 1.5, 0), ("uniform", 0, 1, -0.5, 1, 0), ("uniform", 0, 1, 0, 1, 2), ("uniform", 0, 1, float("nan"), 1, 0)):
        with pytest.raises(ValueError, match="flow time"):
            check_flow_time(*bad)
    flow = dict(time_dim=6, min_period=4e-3, max_period=4.0, time_dist="uniform", dist_a=0.0, dist_b=1.0)
    tm = dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0, stratify=False, name="beta:1.5,1.0")
    assert HeadSpec(flow=flow, flow_time=tm).flow_time == tm and HeadSpec(flow=flow).flow_time is None
    with pytest.raises(ValueError, match="regression"):
        HeadSpec(flow_time=tm)
    with pytest.raises(ValueError, match="flow_noise_draws"):
        HeadSpec(flow=flow, flow_time={**tm, "stratify": True})
    assert HeadSpec(flow=flow, flow_time={**tm, "stratify": True}, draws=2).flow_time["stratify"] is True

    class Recorder:      # apply: the one extra call, right behind set_head_flow
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a, **k: self.calls.append((name, a, k))

    rec = Recorder()
    HeadSpec(flow=flow, flow_time=tm, draws=2).apply(rec)
    assert [c[0] for c in rec.calls] == ["set_head_flow", "set_head_flow_time", "set_head_flow_draws"]
    assert rec.calls[1][2] == dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0, stratify=False)
    rec = Recorder()
    HeadSpec(flow=flow, draws=2).apply(rec)
    assert [c[0] for c in rec.calls] == ["set_head_flow", "set_head_flow_draws"]      # a spec without the setting calls what it called


def _core(**kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=3, **kw)


def test_time_options_on_the_policies_and_the_record(monkeypatch):
    from vla_fastvlm.utils.checkpoint import flow_kwargs
    for k in TIME_ENV:
        monkeypatch.delenv(k, raising=False)
    flow = dict(action_head="flow", flow_time_dim=6, flow_steps=4, flow_seed=9)
    base = {"type": "flow", "steps": 4, "time_dim": 6, "min_period": 4e-3, "max_period": 4.0, "time_dist": "uniform", "dist_a": 0.0, "dist_b": 1.0, "seed": 9}
    plain, pi0 = _core(**flow), _core(**flow, flow_time_dist="pi0")
    assert plain.model.flow_time is None and plain.model.flow_record() == base and plain.model.backbone.head_spec.flow_time is None
    assert pi0.model.flow_time == dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0, stratify=False, name="beta:1.5,1.0")
    assert pi0.model.backbone.head_spec.flow_time == pi0.model.flow_time and pi0.model.flow == plain.model.flow
    # the record: time_dist holds the string, dist_a / dist_b keep their constants, time_range / time_stratify only when set
    assert pi0.model.flow_record() == {**base, "time_dist": "beta:1.5,1.0", "time_range": [0.001, 1.0]}
    beta = _core(**flow, flow_time_dist="beta:2,5")
    assert beta.model.flow_record() == {**base, "time_dist": "beta:2.0,5.0"}
    strat = _core(**flow, flow_time_dist="logit_normal", flow_time_stratify=True, flow_noise_draws=4)
    assert strat.model.flow_record() == {**base, "time_dist": "logit_normal", "time_stratify": True}
    # ... and back: flow_kwargs maps a record without the new keys to what it mapped to, and each policy rebuilds from its own record
    assert flow_kwargs(plain.model.flow_record()) == {"action_head": "flow", "flow_steps": 4, "flow_time_dim": 6, "flow_time_dist": "uniform", "flow_seed": 9}
    assert flow_kwargs(pi0.model.flow_record()) == {"action_head": "flow", "flow_steps": 4, "flow_time_dim": 6, "flow_time_dist": "beta:1.5,1.0", "flow_seed": 9,
                                                    "flow_time_range": (0.001, 1.0)}
    for pol, extra in ((pi0, {}), (beta, {}), (strat, {"flow_noise_draws": 4})):
        again = _core(**flow_kwargs(pol.model.flow_record()), **extra)
        assert again.model.flow_record() == pol.model.flow_record() and again.model.flow_time == pol.model.flow_time
    # a LOAD of a record with strata: without draws (no checkpoint records them) the distribution comes back without strata, with the twin it keeps them
    from vla_fastvlm.utils.checkpoint import strata_need_draws
    kw = flow_kwargs(strat.model.flow_record())
    assert kw["flow_time_stratify"] is True and strata_need_draws(kw)["flow_time_stratify"] is False and kw["flow_time_stratify"] is True
    assert _core(**strata_need_draws(kw)).model.flow_time is None      # (logit-normal on [0, 1] without strata is set_head_flow's own distribution)
    assert strata_need_draws(flow_kwargs(pi0.model.flow_record())) == flow_kwargs(pi0.model.flow_record())
    monkeypatch.setenv("FASTVLA_FLOW_NOISE_DRAWS", "4")
    assert strata_need_draws(kw)["flow_time_stratify"] is True and _core(**strata_need_draws(kw)).model.flow_record() == strat.model.flow_record()
    monkeypatch.delenv("FASTVLA_FLOW_NOISE_DRAWS")
    # refusals on the constructor, before any engine exists
    with pytest.raises(ValueError, match="beta:<alpha>,<beta>"):
        _core(**flow, flow_time_dist="beta")
    with pytest.raises(ValueError, match="flow_time_stratify.*flow_noise_draws"):
        _core(**flow, flow_time_stratify=True)
    with pytest.raises(ValueError, match="flow_time_range.*regression"):
        _core(flow_time_range=(0.0, 0.5))
    with pytest.raises(ValueError, match="needs action_head='flow'"):
        plain_reg = _core()
        plain_reg.model.flow_loss_per_time(None, None, None)
    # the twins reach the constructor, for a flow head only
    monkeypatch.setenv("FASTVLA_FLOW_TIME_DIST", "pi0")
    assert _core(**flow).model.flow_record()["time_dist"] == "beta:1.5,1.0" and _core().model.flow_record() is None


def test_time_options_on_the_lerobot_plugin(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    import dataclasses
    for k in TIME_ENV:
        monkeypatch.delenv(k, raising=False)
    # the registered config gains no field
    assert not [f.name for f in dataclasses.fields(LRConfig) if f.name.startswith("flow_time")]

    def cfg():
        return LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0, chunk_size=3, n_action_steps=1,
                        input_features={"observation.state": PolicyFeature(FeatureType.STATE, (14,)), "observation.image": PolicyFeature(FeatureType.VISUAL, (3, 64, 64))},
                        output_features={ACTION: PolicyFeature(FeatureType.ACTION, (14,))})

    pol = LRPolicy(cfg(), action_head="flow", flow_time_dim=6, flow_seed=9, flow_time_dist="pi0", flow_time_stratify=True, flow_noise_draws=2)
    assert pol.model.flow_time == dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0, stratify=True, name="beta:1.5,1.0")
    rec = pol.model.flow_record()
    assert rec["time_dist"] == "beta:1.5,1.0" and rec["time_range"] == [0.001, 1.0] and rec["time_stratify"] is True and hasattr(pol, "flow_loss_per_time")
    with pytest.raises(ValueError, match="flow_time_dist.*regression"):
        LRPolicy(cfg(), flow_time_dist="pi0")
