"""CPU: the float64 reference of the flow head's higher-order integrators (tests/flow_solver_util.py) against flow_util's Euler sampler and against the exact
linear-Gaussian flow, the fp32 emulation's distance on every case the GPU test uses, and the host side of the option (resolution, setter, record)."""
import pytest
import torch

import flow_solver_util as su
import flow_util as fu
import rtc_util as ru

SOLVER_ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_STEPS", "FASTVLA_FLOW_TIME_DIM", "FASTVLA_FLOW_TIME_DIST", "FASTVLA_FLOW_SOLVER", "FASTVLA_RTC",
              "FASTVLA_FLOW_PREFIX_MAX_DELAY", "FASTVLA_FLOW_NOISE_DRAWS")


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 1)])
def test_euler_tableau_is_flow_utils_euler_sampler(name, B):
    c = fu.sampler_case(name, B)
    E = c["dims"][6]
    for N in (1, 4, 10):
        for kw in ({}, ru.io_kwargs(c, True)):
            args = (c["p"], c["pooled"], c["states"], c["noise"], N, E)
            assert torch.equal(su.rk_sample(*args, "euler", **kw), fu.euler_sample(*args, **kw))
    field, eps, _ = su.toy()
    z = torch.zeros(64, 1)
    assert torch.equal(su.rk_sample({}, z, z, eps, 10, 2, "euler", field=field), fu.euler_sample({}, z, z, eps, 10, 2, field=field))
    # the guided and the prefix variants reduce to their Euler references too
    rc = ru.rtc_case(name, B)
    K, A = rc["dims"][4], rc["dims"][5]
    Y, W = ru.targets(rc["prev"], ru.prefix_weights_ref(K, 0, 1, "exp"), K, A, 1)
    g = (rc["p"], rc["pooled"], rc["states"], rc["noise"], 4, E, Y, W, ru.BETA)
    assert all(torch.equal(a, b) for a, b in zip(su.guided_rk(*g, "euler"), ru.guided_euler(*g)))
    pc = su.prefix_case(name, B)
    import flow_prefix_util as pu
    q = (pc["p"], pc["pooled"], pc["states"], pc["noise"], pc["prev"], pc["delays"], 1, 4, E, K, pc["D"])
    assert all(torch.equal(a, b) for a, b in zip(su.prefix_rk(*q, "euler"), pu.prefix_euler_sample(*q)))


def test_stage_scalars_follow_the_step_times():
    """a stage with c = 1 sees exactly the bits of t_{i + 1}; c = 0 those of t_i"""
    for N in (1, 3, 4, 7, 10):
        ts = fu.step_times(N)
        for i in range(N):
            assert su.stage_time(i, 0.0, N) == ts[i] and su.stage_time(i, 1.0, N) == ts[i + 1]
    assert su.STAGES == {"euler": 1, "midpoint": 2, "heun": 2, "rk4": 4}
    for name, (c, a, b) in su.TABLEAUX.items():
        assert len(a) == len(c) - 1 and len(b) == len(c) and abs(sum(b) - 1.0) < 1e-15 and c[0] == 0.0
        assert all(a[j] == c[j + 1] for j in range(len(a)))      # stage j + 1 is evaluated where its x was carried to


def test_higher_order_solvers_on_the_exact_linear_gaussian_flow():
    """The toy of test_reference_sampler_error_falls_as_one_over_n.  Float64 errors against the exact map, as measured:
        Euler N = 10 6.56e-2;  midpoint N = 5 8.5e-4 (77 x closer), Heun N = 5 4.1e-3 (16 x), RK4 N = 2 3.0e-3 (21 x), each with no more evaluations;
        doubling N from 10, 20, 40 divides the error by at least 3.38 (Heun 10 -> 20).  The field is linear: the ratios are not the textbook orders."""
    euler10 = su.toy_error("euler", 10)
    budget = {"midpoint": 5, "heun": 5, "rk4": 2}
    for solver, N in budget.items():
        err = su.toy_error(solver, N)
        print(f"[flow solver host] {solver} N = {N} ({N * su.STAGES[solver]} evaluations): {err:.3e}, Euler N = 10: {euler10:.3e}, {euler10 / err:.1f} x")
        assert N * su.STAGES[solver] <= 10 and err <= euler10 / 10
    for solver in su.HIGHER:
        errs = {N: su.toy_error(solver, N) for N in (10, 20, 40, 80)}
        print(f"[flow solver host] {solver}:", {k: f"{v:.3e}" for k, v in errs.items()})
        for N in (10, 20, 40):
            assert errs[N] / errs[2 * N] >= 3.0, (solver, errs)


def test_fp32_emulation_stays_within_1e4_of_float64_on_every_gpu_case():
    """the GPU tests' bar is 4 x this distance, as in the flow and RTC tests"""
    worst = {"plain": 0.0, "prefix": 0.0, "guided": 0.0}
    for case in su.plain_cases():
        ref, emu = su.plain_refs(*case)
        assert bool(torch.isfinite(ref).all()) and emu <= 1e-4, (case, emu)
        worst["plain"] = max(worst["plain"], emu)
    for case in su.prefix_cases():
        act, chunk, ea, ec = su.prefix_refs(*case)
        assert bool(torch.isfinite(act).all()) and max(ea, ec) <= 1e-4, (case, ea, ec)
        worst["prefix"] = max(worst["prefix"], ea, ec)
    for case in su.guided_cases():
        act, chunk, ea, ec = su.guided_refs(*case)
        assert bool(torch.isfinite(act).all()) and max(ea, ec) <= 1e-4, (case, ea, ec)
        worst["guided"] = max(worst["guided"], ea, ec)
    print("[flow solver host] worst fp32 emulation distance:", {k: f"{v:.3e}" for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------------------------ the option
def test_flow_solver_option_resolution(monkeypatch):
    from fastvla_hip import _lib
    from vla_fastvlm.fastvla.modeling_fastvla import resolve_flow_options, resolve_flow_solver
    for k in SOLVER_ENV:
        monkeypatch.delenv(k, raising=False)
    assert _lib.FLOW_SOLVERS == {"euler": 0, "midpoint": 1, "heun": 2, "rk4": 3}
    assert resolve_flow_solver(action_head="flow") == "euler" and resolve_flow_solver(action_head="regression") == "euler"
    for name in _lib.FLOW_SOLVERS:
        assert resolve_flow_solver(name, action_head="flow") == name and resolve_flow_solver(name.upper(), action_head="flow") == name
    monkeypatch.setenv("FASTVLA_FLOW_SOLVER", "heun")
    assert resolve_flow_solver(action_head="flow") == "heun"
    assert resolve_flow_solver("rk4", action_head="flow") == "rk4"                      # the argument beats the twin
    assert resolve_flow_solver(action_head="regression") == "euler"                    # the twin is read for a flow head only
    monkeypatch.setenv("FASTVLA_FLOW_SOLVER", "dopri5")
    assert resolve_flow_solver(action_head="regression") == "euler"                    # ... and checked for one only
    with pytest.raises(ValueError, match="FASTVLA_FLOW_SOLVER"):
        resolve_flow_solver(action_head="flow")
    monkeypatch.delenv("FASTVLA_FLOW_SOLVER")
    for bad in ("rk45", "", 3, 1.5):
        with pytest.raises(ValueError, match="flow_solver"):
            resolve_flow_solver(bad, action_head="flow")
    with pytest.raises(ValueError, match="regression"):
        resolve_flow_solver("heun", action_head="regression")
    with pytest.raises(ValueError, match="regression"):
        resolve_flow_solver("euler", action_head="regression")
    # resolve_flow_options() is what it was: no key for the solver, whatever the twin says
    monkeypatch.setenv("FASTVLA_FLOW_SOLVER", "rk4")
    want = dict(time_dim=64, min_period=4e-3, max_period=4.0, time_dist="uniform", dist_a=0.0, dist_b=1.0)
    assert resolve_flow_options() == {"action_head": "regression", "steps": 10, "flow": None}
    assert resolve_flow_options("flow") == {"action_head": "flow", "steps": 10, "flow": want}


def _core(**kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=3, **kw)


def test_flow_solver_on_the_policies_setter_and_record(monkeypatch):
    """no GPU: the argument, the twin, the refusals, the setter's rule and the checkpoint record on both surfaces"""
    from vla_fastvlm.utils.checkpoint import flow_kwargs
    for k in SOLVER_ENV:
        monkeypatch.delenv(k, raising=False)
    flow = dict(action_head="flow", flow_time_dim=6, flow_steps=4, flow_seed=9)
    euler, heun = _core(**flow), _core(**flow, flow_solver="heun")
    assert euler.flow_solver == "euler" and heun.flow_solver == "heun" and heun.flow_steps == 4
    assert heun.model.backbone.head_spec.solver == "heun" and heun.model.backbone.head_spec.solver_rows and not euler.model.backbone.head_spec.solver_rows
    # the record: "solver" only when it is not Euler; flow_kwargs maps it back; an Euler run writes the record it wrote
    base = {"type": "flow", "steps": 4, "time_dim": 6, "min_period": 4e-3, "max_period": 4.0, "time_dist": "uniform", "dist_a": 0.0, "dist_b": 1.0, "seed": 9}
    assert euler.model.flow_record() == base and heun.model.flow_record() == {**base, "solver": "heun"}
    assert flow_kwargs(euler.model.flow_record()) == {"action_head": "flow", "flow_steps": 4, "flow_time_dim": 6, "flow_time_dist": "uniform", "flow_seed": 9}
    assert flow_kwargs(heun.model.flow_record())["flow_solver"] == "heun"
    again = _core(**flow_kwargs(heun.model.flow_record()))
    assert again.flow_solver == "heun" and again.model.flow_record() == heun.model.flow_record()
    # a policy built with a higher-order solver switches among all four (Euler included) at any time; the record follows
    for name in ("rk4", "euler", "midpoint", "heun"):
        heun.flow_solver = name
        assert heun.flow_solver == name and heun.model.backbone.head_spec.solver == name and heun.model.backbone.head_spec.solver_rows
        assert heun.model.flow_record().get("solver") == (None if name == "euler" else name)
    with pytest.raises(ValueError, match="flow_solver"):
        heun.flow_solver = "rk5"
    assert heun.flow_solver == "heun"
    # a policy built with Euler: the rows were not reserved, and the message names the remedy
    with pytest.raises(ValueError, match="build the policy with flow_solver"):
        euler.flow_solver = "rk4"
    euler.flow_solver = "euler"
    assert euler.flow_solver == "euler"
    # the twin, for a flow head only; the argument beats it
    monkeypatch.setenv("FASTVLA_FLOW_SOLVER", "midpoint")
    assert _core(**flow).flow_solver == "midpoint" and _core(**flow, flow_solver="euler").flow_solver == "euler"
    reg = _core()
    assert reg.flow_solver == "euler" and reg.model.flow_record() is None
    with pytest.raises(ValueError, match="regression"):
        _core(flow_solver="heun")
    with pytest.raises(ValueError, match="regression"):
        reg.flow_solver = "heun"
    monkeypatch.setenv("FASTVLA_FLOW_SOLVER", "nonsense")
    assert _core().flow_solver == "euler"
    with pytest.raises(ValueError, match="FASTVLA_FLOW_SOLVER"):
        _core(**flow)


def test_flow_solver_on_the_lerobot_plugin(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    import dataclasses
    for k in SOLVER_ENV:
        monkeypatch.delenv(k, raising=False)
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}

    def make(**kw):
        cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=4, n_action_steps=2,
                       output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(5,))}, dropout=0.0)
        return LRPolicy(cfg, **kw)

    flow = dict(action_head="flow", flow_time_dim=6, flow_steps=5, flow_seed=11)
    pol = make(**flow, flow_solver="rk4")
    assert pol.flow_solver == "rk4" and pol.model.flow_record()["solver"] == "rk4"
    pol.flow_solver = "euler"
    assert pol.flow_solver == "euler" and "solver" not in pol.model.flow_record()
    assert not any("solver" in f.name for f in dataclasses.fields(LRConfig))      # the registered config gains no field
    with pytest.raises(ValueError, match="build the policy with flow_solver"):
        make(**flow).flow_solver = "heun"
    with pytest.raises(ValueError, match="regression"):
        make(flow_solver="midpoint")
    monkeypatch.setenv("FASTVLA_FLOW_SOLVER", "heun")
    assert make(**flow).flow_solver == "heun" and make().flow_solver == "euler"
