"""CPU: the flow-matching head's reference itself (tests/flow_util.py) and the host-side option handling.  The GPU tests (tests/test_gpu_flow.py) compare the
kernels with this reference; here the reference is held against facts that do not depend on it: an exact velocity field, the moments of a normal, the
distance between its fp32 and float64 forms on every input the GPU sampler test uses, and the bimodal toy with thresholds stricter than the GPU test's."""
import numpy as np
import pytest
import torch

import flow_util as fu


def test_reference_sampler_error_falls_as_one_over_n():
    """a ~ N(m, s^2 I) and eps ~ N(0, I) independent: x_t = t eps + (1 - t) a is Gaussian, and the exact field is linear in x,
        v(x, t) = E[eps - a | x_t = x] = -m + (t - (1 - t) s^2) / (t^2 + (1 - t)^2 s^2) (x - (1 - t) m),
    whose flow maps x_1 = eps to m + s eps exactly.  Euler is first order: doubling N halves the error."""
    m, s = torch.tensor([0.7, -1.2, 0.3]).double(), 0.5
    eps = torch.randn(64, 3, generator=torch.Generator().manual_seed(0)).double()

    def field(x, t):
        return -m + (t - (1 - t) * s * s) / (t * t + (1 - t) ** 2 * s * s) * (x - (1 - t) * m)

    exact = m + s * eps
    errs = {N: float((fu.euler_sample({}, torch.zeros(64, 1), torch.zeros(64, 1), eps, N, 2, field=field) - exact).norm() / exact.norm()) for N in (10, 20, 40, 80, 160)}
    print("[flow host] Euler error against the exact flow:", {k: f"{v:.3e}" for k, v in errs.items()})
    for N in (10, 20, 40, 80):
        assert 1.6 <= errs[N] / errs[2 * N] <= 2.4, errs
    assert errs[160] < 5e-3


def test_reference_box_muller_moments_and_stream():
    n, _ = fu.draw_normals(512, 700, seed=9, offset=3)
    N = n.size
    assert abs(n.mean()) <= 4 / np.sqrt(N) and abs(n.std() - 1) <= 4 / np.sqrt(2 * N)
    assert abs((n ** 3).mean()) <= 4 * np.sqrt(15 / N) and abs((n ** 4).mean() - 3) <= 4 * np.sqrt(96 / N)
    # the four normals of a group are the two Box-Muller pairs of ONE Philox block: uncorrelated, and rows / offsets / seeds give other values
    assert abs(np.corrcoef(n[:, 0], n[:, 1])[0, 1]) < 0.2 and abs(np.corrcoef(n[:, 0], n[:, 2])[0, 1]) < 0.2
    assert not np.array_equal(n[0], n[1]) and not np.array_equal(n, fu.draw_normals(512, 700, seed=9, offset=4)[0])
    assert np.array_equal(n[:3, :21], fu.draw_normals(3, 21, seed=9, offset=3)[0])            # a function of (row, element) only
    t = fu.draw_t_uniform(4096, seed=9, offset=3)
    assert t.dtype == np.float32 and 0 <= t.min() and t.max() < 1 and abs(t.mean() - 0.5) < 4 / np.sqrt(12 * 4096)
    tl = fu.draw_t_logit_normal(4096, 9, 3, 0.0, 1.0)
    assert 0 < tl.min() and tl.max() < 1 and abs(np.median(tl) - 0.5) < 0.05


def test_time_embedding_definition():
    w = fu.flow_freqs(64)
    assert w.dtype == np.float32 and w.shape == (32,)
    np.testing.assert_allclose(w[0], 2 * np.pi / 4e-3, rtol=1e-6)
    np.testing.assert_allclose(w[-1], 2 * np.pi / 4.0, rtol=1e-6)
    np.testing.assert_allclose(w[1:] / w[:-1], (4e-3 / 4.0) ** (1 / 31), rtol=1e-5)        # geometric periods
    assert fu.flow_freqs(2).shape == (1,)
    ph = fu.phi_ref(np.array([0.0, 1.0], dtype=np.float32), w)
    assert ph.shape == (2, 64) and np.all(ph[0, :32] == 0) and np.all(ph[0, 32:] == 1)
    assert float(fu.phi_args(np.array([1.0], dtype=np.float32), w).max()) > 1500              # why the kernel needs sinf / cosf


@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_fp32_emulation_stays_within_1e_4_of_float64_on_every_gpu_sampler_input(name):
    """the GPU sampler's bar is 4 x this distance: it may not be loose"""
    worst = 0.0
    for B in fu.SAMPLER_BATCHES:
        case = fu.sampler_case(name, B)
        for io in (False, True):
            for N in fu.SAMPLER_STEPS:
                _, emu = fu.sampler_refs(case, N, io)
                worst = max(worst, emu)
                assert 0 < emu <= 1e-4, (name, B, N, io, emu)
    print(f"[flow host {name}] fp32 emulation against float64, worst row / rms row norm: {worst:.3e}")


def test_bimodal_toy_on_the_reference():
    flow, reg = fu.bimodal_reference(True), fu.bimodal_reference(False)
    print(f"[flow host bimodal] flow: {flow}; regression: {reg}")
    assert flow["plus"] >= 0.35 and flow["minus"] >= 0.35 and flow["mean_abs"] >= 0.85
    assert reg["mean_abs"] <= 0.2


# ------------------------------------------------------------------------------------------------------------------ options, records, refusals
FLOW_ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_STEPS", "FASTVLA_FLOW_TIME_DIM", "FASTVLA_FLOW_TIME_DIST")


def test_flow_option_resolution(monkeypatch):
    from vla_fastvlm.fastvla.modeling_fastvla import resolve_flow_options
    for k in FLOW_ENV:
        monkeypatch.delenv(k, raising=False)
    assert resolve_flow_options() == {"action_head": "regression", "steps": 10, "flow": None}            # the default asks for nothing new
    want = dict(time_dim=64, min_period=4e-3, max_period=4.0, time_dist="uniform", dist_a=0.0, dist_b=1.0)
    assert resolve_flow_options("flow") == {"action_head": "flow", "steps": 10, "flow": want}
    assert resolve_flow_options("flow", 4, 6, "logit_normal") == {"action_head": "flow", "steps": 4, "flow": {**want, "time_dim": 6, "time_dist": "logit_normal"}}
    monkeypatch.setenv("FASTVLA_ACTION_HEAD", "flow")
    monkeypatch.setenv("FASTVLA_FLOW_STEPS", "7")
    monkeypatch.setenv("FASTVLA_FLOW_TIME_DIM", "8")
    monkeypatch.setenv("FASTVLA_FLOW_TIME_DIST", "logit_normal")
    assert resolve_flow_options() == {"action_head": "flow", "steps": 7, "flow": {**want, "time_dim": 8, "time_dist": "logit_normal"}}
    got = resolve_flow_options(flow_steps=3, flow_time_dim=10, flow_time_dist="uniform")                  # the argument beats the twin
    assert got["steps"] == 3 and got["flow"]["time_dim"] == 10 and got["flow"]["time_dist"] == "uniform"
    assert resolve_flow_options("regression")["flow"] is None
    monkeypatch.setenv("FASTVLA_ACTION_HEAD", "regression")          # a regression head neither reads nor checks the flow twins
    monkeypatch.setenv("FASTVLA_FLOW_TIME_DIM", "7")
    monkeypatch.setenv("FASTVLA_FLOW_STEPS", "zero")
    assert resolve_flow_options() == {"action_head": "regression", "steps": 10, "flow": None}
    with pytest.raises(ValueError):
        resolve_flow_options("flow")
    for k in FLOW_ENV:
        monkeypatch.delenv(k, raising=False)
    for bad in (dict(action_head="diffusion"), dict(action_head="flow", flow_steps=0), dict(action_head="flow", flow_steps=2.5), dict(action_head="flow", flow_time_dim=7),
                dict(action_head="flow", flow_time_dim=0), dict(action_head="flow", flow_time_dim=-4), dict(action_head="flow", flow_time_dist="beta")):
        with pytest.raises(ValueError):
            resolve_flow_options(**bad)


def test_flow_policy_modules_record_and_mismatched_loads(monkeypatch):
    """no GPU: the module tree of a flow policy, its noise-stream offsets, the checkpoint record and the two mismatched-load messages"""
    from types import SimpleNamespace
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    from vla_fastvlm.utils.checkpoint import check_fusion_width, flow_kwargs
    for k in FLOW_ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0)
    reg = FastVLAPolicy(cfg, chunk_size=3)
    flow = FastVLAPolicy(cfg, chunk_size=3, action_head="flow", flow_time_dim=6, flow_steps=4, flow_seed=9)
    feat = reg.model.backbone.output_dim
    assert reg.action_head == "regression" and reg.model.flow is None and reg.model.flow_record() is None and reg.model.fusion[0].in_features == feat + 48
    assert flow.model.fusion[0].in_features == feat + 48 + 3 * 14 + 6 and list(flow.state_dict()) == list(reg.state_dict())      # the same 12 keys
    assert flow.model.flow_record() == {"type": "flow", "steps": 4, "time_dim": 6, "min_period": 4e-3, "max_period": 4.0, "time_dist": "uniform", "dist_a": 0.0,
                                        "dist_b": 1.0, "seed": 9}
    assert flow_kwargs(flow.model.flow_record()) == {"action_head": "flow", "flow_steps": 4, "flow_time_dim": 6, "flow_time_dist": "uniform", "flow_seed": 9}
    assert flow_kwargs(None) == {"action_head": "regression"}
    for key, val in (("min_period", 1e-3), ("max_period", 8.0), ("dist_a", 0.5), ("dist_b", 2.0)):      # a record written with another embedding / distribution
        with pytest.raises(ValueError, match=key):
            flow_kwargs({**flow.model.flow_record(), key: val})
    flow.flow_steps = 12
    assert flow.model.flow_steps == 12
    with pytest.raises(ValueError):
        flow.flow_steps = 0
    # four disjoint offset ranges under one seed; the evaluation index restarts when the mode is set
    m = flow.model
    assert m.flow_train_draw(3, 1) == (9, (3 << 16) + 1) and m.flow_train_draw(3, 1) == m.flow_train_draw(3, 1)
    assert m.flow_sample_draw()[1] == (1 << 62) + 1 and m.flow_sample_draw()[1] == (1 << 62) + 2
    assert m.flow_eval_draw()[1] == (1 << 61) + 1 and m.flow_eval_draw()[1] == (1 << 61) + 2
    flow.eval()
    assert m.flow_eval_draw()[1] == (1 << 61) + 1
    assert m.flow_loss_draw()[1] == (1 << 60) + 1
    # the head's layout is fixed before the engine exists
    assert flow.model.backbone.head_spec.flow == m.flow and reg.model.backbone.head_spec.flow is None
    for pol, other in ((reg, flow), (flow, reg)):
        with pytest.raises(ValueError) as ei:
            check_fusion_width({"model.fusion.0.weight": other.model.fusion[0].weight.detach()}, pol, "ckpt")
        msg = str(ei.value)
        assert "model.fusion.0.weight" in msg and str(tuple(other.model.fusion[0].weight.shape)) in msg and str(tuple(pol.model.fusion[0].weight.shape)) in msg
        assert f"action_head='{pol.action_head}'" in msg
    check_fusion_width({"model.fusion.0.weight": flow.model.fusion[0].weight.detach()}, flow)
    check_fusion_width({}, SimpleNamespace(model=reg.model))


def test_lora_host_layout_follows_the_flow_width():
    from fastvla_hip import arch, lora
    model = arch.preset("tiny")
    plain, _ = lora.lora_layout(model, 4, state_dim=14, action_dim=12, hidden_dim=32, fusion_dim=48)
    wide, _ = lora.lora_layout(model, 4, state_dim=14, action_dim=12, hidden_dim=32, fusion_dim=48, flow_time_dim=6)
    assert plain[4]["cols"] == model.llm.hidden + 32 and wide[4]["cols"] == model.llm.hidden + 32 + 12 + 6
    assert [t["name"] for t in plain] == [t["name"] for t in wide] and all(a["numel"] == b["numel"] for i, (a, b) in enumerate(zip(plain, wide)) if i != 4)
