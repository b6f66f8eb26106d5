"""CPU: the one path of a policy option -- constructor keyword or FASTVLA_* twin -> resolve_policy_options -> PolicyOptions -> HeadSpec -> the ordered
set_head_* calls of HeadSpec.apply.  No engine is built: the engine side is a stub that records what it is told."""
import dataclasses
import os

import pytest
import torch


@pytest.fixture(autouse=True)
def _no_twins(monkeypatch):
    for k in [k for k in os.environ if k.startswith("FASTVLA_")]:
        monkeypatch.delenv(k)


def _core(K=3, n=2, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", state_dim=6, action_dim=5, hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K,
                         n_action_steps=n, **kw)


def _plugin(K=3, n=2, **kw):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, input_features=feats, chunk_size=K, n_action_steps=n,
                   output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(5,))}, dropout=0.0)
    return LRPolicy(cfg, **kw)


SURFACES = (_core, _plugin)
FLOW = dict(action_head="flow", flow_steps=2, flow_time_dim=6)
DIM_W, STEP_W = [1.0, 1.0, 1.0, 1.0, 4.0], [1.0, 0.5, 0.25]
# (chunk_size, n_action_steps, keywords, twins set for BOTH ways of asking: the loss kind has no keyword on the LeRobot surface)
TABLE = {
    "off": (1, 1, {}, {}),
    "chunks": (3, 2, {}, {}),
    "loss weights": (3, 2, dict(action_dim_weights=DIM_W, action_step_weights="discount:0.5"), {}),
    "temporal ensembling": (3, 1, dict(temporal_ensemble_coeff=0.1), {}),
    "flow head": (3, 2, dict(**FLOW, flow_time_dist="logit_normal", flow_seed=7), {}),
    "noise draws": (3, 2, dict(**FLOW, flow_noise_draws=2), {}),
    "rtc guidance": (3, 2, dict(**FLOW, rtc=True, rtc_schedule="linear", rtc_max_guidance_weight=3.0, rtc_execution_horizon=2), {}),
    "prefix": (3, 2, dict(**FLOW, flow_prefix_max_delay=1, flow_prefix_delay_dist="exp", flow_prefix_delay_rate=0.25), {}),
    "solver": (3, 2, dict(**FLOW, flow_solver="heun"), {}),
    "samples": (3, 2, dict(**FLOW, flow_samples=3, flow_select="coherent", flow_coherence_decay=0.25), {}),
    "everything": (3, 2, dict(**FLOW, flow_noise_draws=2, flow_prefix_max_delay=1, rtc=True, rtc_method="prefix", flow_solver="heun", flow_samples=3,
                              flow_select="coherent", action_dim_weights=DIM_W, action_step_weights=STEP_W),
                   {"FASTVLA_ACTION_LOSS": "smooth_l1", "FASTVLA_ACTION_LOSS_BETA": "0.5"}),
}
NO_TWIN = ("flow_seed",)      # (chunk_size and n_action_steps have twins, but the LeRobot surface takes them from its config, always)
# a twin for every keyword of the "everything" row that says something else
CONTRADICTING = {"FASTVLA_ACTION_HEAD": "regression", "FASTVLA_FLOW_STEPS": "9", "FASTVLA_FLOW_TIME_DIM": "12", "FASTVLA_FLOW_NOISE_DRAWS": "5",
                 "FASTVLA_FLOW_PREFIX_MAX_DELAY": "2", "FASTVLA_RTC": "0", "FASTVLA_RTC_METHOD": "guidance", "FASTVLA_FLOW_SOLVER": "rk4", "FASTVLA_FLOW_SAMPLES": "7",
                 "FASTVLA_FLOW_SELECT": "first", "FASTVLA_ACTION_DIM_WEIGHTS": "2,2,2,2,2", "FASTVLA_ACTION_STEP_WEIGHTS": "discount:0.9"}


def _twin(key, value):
    text = "1" if value is True else ",".join(str(x) for x in value) if isinstance(value, list) else str(value)
    return "FASTVLA_" + key.upper(), text


def _alike(a, b):
    assert a.options == b.options and a.model.backbone.head_spec == b.model.backbone.head_spec
    for name in ("temporal_ensemble_coeff", "action_head", "flow_noise_draws", "flow_prefix", "flow_samples", "flow_select", "rtc", "flow_steps", "flow_solver"):
        assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("row", list(TABLE))
def test_both_surfaces_resolve_alike(monkeypatch, row):
    from vla_fastvlm.fastvla.options import PolicyOptions
    K, n, kw, env = TABLE[row]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    core, plug = _core(K, n, **kw), _plugin(K, n, **kw)
    _alike(core, plug)
    assert isinstance(core.options, PolicyOptions) and core.model.backbone._engine is None and plug.model.backbone._engine is None
    assert core.n_action_steps == n and core.options.chunk["chunk_size"] == K and core.model.backbone.head_spec.dims["action_dim"] == 5 * K
    if row == "off":
        assert core.options == dataclasses.replace(PolicyOptions()) and core.model.backbone.head_spec == type(core.model.backbone.head_spec)(
            dims=dict(state_dim=6, action_dim=5, hidden_dim=48, fusion_dim=64))
    if row == "everything":
        o, spec = core.options, core.model.backbone.head_spec
        assert (o.chunk["loss"], o.chunk["beta"], o.noise_draws, o.solver, o.samples, o.select) == ("smooth_l1", 0.5, 2, "heun", 3, "coherent")
        assert o.rtc == {"method": "prefix", "prefix_steps": 1, "max_delay": 1} and o.prefix["max_delay"] == 1
        assert spec.loss == dict(kind="smooth_l1", beta=0.5, chunk=3) and spec.loss_weights == {"dim": DIM_W, "step": STEP_W} and spec.solver_rows
        assert spec.samples == dict(max_samples=3, step_weights=[1.0, 0.5, 0.25]) and spec.guidance is None and spec.draws == 2
    # the same through the twins: every option that has one
    for k, v in kw.items():
        if k not in NO_TWIN:
            monkeypatch.setenv(*_twin(k, v))
    seed = {k: v for k, v in kw.items() if k in NO_TWIN}
    for make in SURFACES:
        _alike(make(K, n, **seed), core)
    # an explicit argument beats a twin that says something else
    if row == "everything":
        for k, v in CONTRADICTING.items():
            monkeypatch.setenv(k, v)
        for make in SURFACES:
            _alike(make(K, n, **kw), core)


# (the earlier resolver's bad setting, its message; the later resolver's bad setting, its message): six adjacent pairs pin the seven-step order
CHUNK_BAD = (dict(action_dim_weights=[-1.0]), "action_dim_weights must be finite and >= 0")
FLOW_BAD = (dict(flow_time_dim=5), "flow_time_dim must be a positive even integer")
DRAWS_BAD = (dict(flow_noise_draws=17), "flow_noise_draws must be an integer 1 .. 16. Got flow_noise_draws=17")
SOLVER_BAD = (dict(flow_solver="rk5"), "flow_solver must be 'euler', 'midpoint', 'heun' or 'rk4'. Got flow_solver='rk5'")
PREFIX_BAD = (dict(flow_prefix_max_delay=3), "flow_prefix_max_delay=3 must be below chunk_size=3")
RTC_BAD = (dict(rtc=True, rtc_method="warp"), "rtc_method must be 'guidance' or 'prefix', got 'warp'")
SAMPLES_BAD = (dict(flow_samples=17), "flow_samples must be an integer 1 .. 16, got 17")
ORDER = (CHUNK_BAD, FLOW_BAD, DRAWS_BAD, SOLVER_BAD, PREFIX_BAD, RTC_BAD, SAMPLES_BAD)


@pytest.mark.parametrize("i", range(6))
def test_first_error_wins(i):
    import re
    from vla_fastvlm.fastvla.options import resolve_policy_options
    (first, first_msg), (second, second_msg) = ORDER[i], ORDER[i + 1]
    makers = SURFACES + (lambda K, n, **kw: resolve_policy_options(chunk_size=K, n_action_steps=n, **kw),)
    for make in makers:
        with pytest.raises(ValueError, match=re.escape(second_msg)):      # (the later setting IS refused on its own)
            make(3, 2, action_head="flow", **second)
        with pytest.raises(ValueError, match=re.escape(first_msg)):
            make(3, 2, action_head="flow", **first, **second)


class Recorder:
    """stands in for a FastVLAEngine: records (method name, positional arguments, keyword arguments) of every set_* call"""

    def __init__(self, **mirrors):
        self.calls = []
        self.__dict__.update(mirrors)

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a, **k: self.calls.append((name, a, k))

    def close(self):
        pass


DIMS = dict(state_dim=6, action_dim=15, hidden_dim=48, fusion_dim=64)
FLOW_SPEC = dict(time_dim=6, min_period=4e-3, max_period=4.0, time_dist="uniform", dist_a=0.0, dist_b=1.0)
LOSS = dict(kind="smooth_l1", beta=0.5, chunk=3)
GUIDANCE = dict(step_weights=[1.0, 0.5, 0.0], max_guidance_weight=3.0)
SAMPLES = dict(max_samples=3, step_weights=[1.0, 0.5, 0.25])


def _everything():
    from fastvla_hip.head_spec import HeadSpec
    from fastvla_hip.prefix import check_prefix_config
    return HeadSpec(dims=DIMS, loss=LOSS, loss_weights={"dim": DIM_W, "step": None}, flow=FLOW_SPEC, prefix=check_prefix_config(1, action_head="flow", chunk_size=3),
                    draws=2, guidance=GUIDANCE, samples=SAMPLES, solver="heun")


def test_replay_order():
    from fastvla_hip.head_spec import HeadSpec

    def replay(spec):
        rec = Recorder()
        spec.apply(rec)
        return rec.calls

    loss_calls = [("set_head_loss", (), LOSS), ("set_head_loss_weights", (DIM_W, None), {})]
    assert replay(HeadSpec(dims=DIMS)) == [] and replay(HeadSpec()) == []
    assert replay(HeadSpec(dims=DIMS, loss=LOSS, loss_weights={"dim": DIM_W, "step": None})) == loss_calls
    assert replay(HeadSpec(dims=DIMS, flow=FLOW_SPEC)) == [("set_head_flow", (), FLOW_SPEC)]
    assert replay(_everything()) == [
        ("set_head_flow", (), FLOW_SPEC),
        ("set_head_flow_prefix", (3, 1), dict(thresholds=[1 << 23, 1 << 24], dist="uniform", rate=0.0)),
        ("set_head_flow_draws", (2,), {}),
        ("set_head_flow_guidance", (), GUIDANCE),
        ("set_head_flow_samples", (), SAMPLES),
        ("set_head_flow_solver", ("heun",), {}),
        ("set_head_flow_solver", ("heun",), {}),
    ] + loss_calls
    back = dataclasses.replace(HeadSpec(dims=DIMS, flow=FLOW_SPEC, solver="heun"), solver="euler")      # built with heun, switched to euler: the rows stay reserved
    assert back.solver == "euler" and back.solver_rows
    assert replay(back) == [("set_head_flow", (), FLOW_SPEC), ("set_head_flow_solver", ("midpoint",), {}), ("set_head_flow_solver", ("euler",), {})]
    assert replay(HeadSpec(dims=DIMS, flow=FLOW_SPEC, guidance=GUIDANCE)) == [("set_head_flow", (), FLOW_SPEC), ("set_head_flow_guidance", (), GUIDANCE)]


def test_head_spec_refusals():
    """the cross-field refusals, once, at construction: with the texts the layers below the resolvers used"""
    from fastvla_hip.head_spec import HeadSpec
    from fastvla_hip.prefix import check_prefix_config
    px = check_prefix_config(1, action_head="flow", chunk_size=3)
    for kw, msg in ((dict(prefix=px), r"flow_prefix_max_delay=1 needs action_head='flow' and the head's chunk_size=1"),
                    (dict(flow=FLOW_SPEC, prefix=px, loss=dict(kind="mse", beta=1.0, chunk=5)), r"flow_prefix_max_delay=1 needs action_head='flow' and the head's chunk_size=5"),
                    (dict(draws=2), r"flow_noise_draws=2 needs action_head='flow' \(the regression head has no noise to draw\)"),
                    (dict(solver="heun"), r"flow_solver='heun' needs action_head='flow' \(the regression head integrates nothing\)"),
                    (dict(samples=SAMPLES), r"flow_samples=3 / flow_select=None need action_head='flow'"),
                    (dict(flow=FLOW_SPEC, solver="rk5"), "flow_solver must be one of"), (dict(flow=FLOW_SPEC, draws=17), "flow_noise_draws must be an integer 1 .. 16"),
                    (dict(loss=dict(kind="huber", beta=1.0, chunk=1)), "unknown action loss 'huber'"), (dict(loss=dict(kind="mse", beta=1.0, chunk=4)), "does not divide"),
                    (dict(loss_weights={"dim": [1.0, 2.0], "step": None}), "action_dim_weights must have 15 values, got 2")):
        with pytest.raises(ValueError, match=msg):
            HeadSpec(**{"dims": DIMS, **kw})


def test_late_changes():
    bb = _core(**FLOW).model.backbone
    spec = _everything()
    bb.configure_head(spec)
    assert bb.head_spec is spec and bb._engine is None
    eng = bb._engine = Recorder(head_flow_solver="heun", head_flow_guidance=dict(chunk=3))
    try:
        # a built engine refuses what its layout and workspaces were sized by ...
        for change, match in ((dict(flow={**FLOW_SPEC, "time_dim": 8}), r"configure_head_flow: the engine is already built \(the head's layout and the workspace depend on the mode\)"),
                              (dict(prefix=None), r"configure_head_flow_prefix: the engine is already built \(the head's layout and the workspace depend on the mode\)"),
                              (dict(draws=3), r"configure_head_flow_draws: the engine is already built \(the saved activations and the workspaces depend on the number of draws\)"),
                              (dict(samples=None), r"configure_head_flow_samples: the engine is already built \(the sampler's rows in the workspace depend on the number of samples\)")):
            with pytest.raises(RuntimeError, match=match):
                bb.configure_head(dataclasses.replace(spec, **change))
        assert bb.head_spec is spec and bb._engine is eng and eng.calls == []
        # ... and is told the four settings that may change at once
        bb.configure_head_loss("l1", 2.0, 3)
        assert eng.calls == [("set_head_loss", (), dict(kind="l1", beta=2.0, chunk=3))] and bb.head_spec.loss_weights == {"dim": DIM_W, "step": None}
        bb.configure_head_loss_weights(None, STEP_W)
        assert eng.calls[-1] == ("set_head_loss_weights", (None, STEP_W), {}) and bb.head_spec.loss_weights == {"dim": None, "step": STEP_W}
        bb.configure_head_loss_weights()
        assert eng.calls[-1] == ("set_head_loss_weights", (None, None), {}) and bb.head_spec.loss_weights is None
        with pytest.raises(ValueError, match="action_step_weights must have 3 values, got 2"):
            bb.configure_head_loss_weights(None, [1.0, 2.0])
        new = dict(step_weights=[0.0, 1.0, 1.0], max_guidance_weight=2.0)
        bb.configure_head_flow_guidance(new)
        assert eng.calls[-1] == ("set_head_flow_guidance", (), new) and bb.head_spec.guidance == new
        bb.configure_head_flow_guidance(None)      # (the engine holds one: it is switched off)
        assert eng.calls[-1] == ("set_head_flow_guidance", (), {"step_weights": None}) and bb.head_spec.guidance is None
        eng.head_flow_guidance, n = None, len(eng.calls)
        bb.configure_head_flow_guidance(None)      # (off on both sides: nothing to tell)
        assert len(eng.calls) == n
        # the solver: told only when one side is not Euler
        bb.configure_head_flow_solver("euler")
        assert eng.calls[-1] == ("set_head_flow_solver", ("euler",), {}) and bb.head_spec.solver == "euler" and bb.head_spec.solver_rows
        eng.head_flow_solver, n = "euler", len(eng.calls)
        bb.configure_head_flow_solver("EULER")
        assert len(eng.calls) == n and bb.head_spec.solver == "euler"
        bb.configure_head_flow_solver("rk4")
        assert eng.calls[-1] == ("set_head_flow_solver", ("rk4",), {}) and bb.head_spec.solver == "rk4"
        with pytest.raises(ValueError, match="flow_solver must be one of"):
            bb.configure_head_flow_solver("rk5")
        # a new chunk length drops the weights (sized for the old one) and re-tiles the folded statistics
        bb.configure_head_loss_weights(DIM_W, STEP_W)
        bb.set_io_normalization(state_mean=torch.zeros(6), state_std=torch.ones(6), action_mean=torch.arange(3.0), action_std=torch.ones(3))
        n = len(eng.calls)
        bb.configure_head_loss("l1", 2.0, 3)      # (the same length: the weights stay, nothing is re-tiled)
        assert [c[0] for c in eng.calls[n:]] == ["set_head_loss"] and bb.head_spec.loss_weights == {"dim": DIM_W, "step": STEP_W}
        n = len(eng.calls)
        bb.configure_head_loss("mse", 1.0, 5)      # (the spec has a prefix of 3 steps: this setter checks the loss alone, the engine refuses the rest)
        assert [c[0] for c in eng.calls[n:]] == ["set_head_loss", "set_io_norm"] and bb.head_spec.loss_weights is None
        assert eng.calls[n][2] == dict(kind="mse", beta=1.0, chunk=5) and torch.equal(eng.calls[n + 1][2]["action_mean"], torch.arange(3.0).repeat(5))
        # a spec with the same layout is taken: the engine is rebuilt on the next use
        bb.configure_head_loss("mse", 1.0, 3)
        bb.configure_head(dataclasses.replace(bb.head_spec, solver="euler"))
        assert bb._engine is None
    finally:
        bb._engine = None
    # the widths alone: a plain regression head (what a caller that builds a backbone by hand passes)
    bb.configure_head(state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64)
    assert bb.head_spec == type(spec)(dims=dict(state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64)) and bb.head_spec.flow is None


def test_the_picker(monkeypatch):
    from vla_fastvlm.fastvla import modeling_fastvla, options
    from vla_fastvlm.fastvla.options import pick, resolve_flow_samples, resolve_prefix_options
    assert modeling_fastvla.resolve_flow_samples is resolve_flow_samples and modeling_fastvla.parse_weight_list is options.parse_weight_list
    assert pick(None, "FASTVLA_X", int, 4) == 4 and pick(0, "FASTVLA_X", int, 4) == 0
    monkeypatch.setenv("FASTVLA_X", " 12 ")
    assert pick(None, "FASTVLA_X", int, 4) == 12 and pick(7, "FASTVLA_X", int, 4) == 7 and pick(None, "FASTVLA_X", int, 4, read=False) == 4
    # a twin the cast refuses, three ways: the cast's own error escapes ...
    monkeypatch.setenv("FASTVLA_X", "many")
    with pytest.raises(ValueError, match=r"invalid literal for int\(\)"):
        pick(None, "FASTVLA_X", int, 4)
    assert pick(None, "FASTVLA_X", int, 4, read=False) == 4
    with pytest.raises(ValueError, match="^FASTVLA_X: 'many' does not go through int$"):
        pick(None, "FASTVLA_X", int, 4, error=lambda env, raw, cast: f"{env}: {raw!r} does not go through {cast.__name__}")
    monkeypatch.setenv("FASTVLA_CHUNK_SIZE", "many")
    with pytest.raises(ValueError, match=r"invalid literal for int\(\)"):
        options.resolve_chunk_options()
    # ... "an integer" / "a number", with both settings named ...
    monkeypatch.setenv("FASTVLA_FLOW_SAMPLES", "many")
    with pytest.raises(ValueError, match=r"^FASTVLA_FLOW_SAMPLES must be an integer, got FASTVLA_FLOW_SAMPLES='many' \(action_head='flow'\)$"):
        resolve_flow_samples(action_head="flow", chunk_size=3)
    assert resolve_flow_samples(action_head="regression", chunk_size=3)["samples"] == 1      # (read for a flow head only)
    monkeypatch.setenv("FASTVLA_FLOW_SAMPLES", "2")
    monkeypatch.setenv("FASTVLA_FLOW_COHERENCE_DECAY", "half")
    with pytest.raises(ValueError, match=r"^FASTVLA_FLOW_COHERENCE_DECAY must be a number, got FASTVLA_FLOW_COHERENCE_DECAY='half' \(action_head='flow'\)$"):
        resolve_flow_samples(action_head="flow", chunk_size=3)
    # ... and the cast's name
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_MAX_DELAY", "two")
    with pytest.raises(ValueError, match="^FASTVLA_FLOW_PREFIX_MAX_DELAY must be int, got 'two'$"):
        resolve_prefix_options(action_head="flow", chunk_size=3)
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_MAX_DELAY", "2")
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_DELAY_RATE", "fast")
    with pytest.raises(ValueError, match="^FASTVLA_FLOW_PREFIX_DELAY_RATE must be float, got 'fast'$"):
        resolve_prefix_options(action_head="flow", chunk_size=3)
