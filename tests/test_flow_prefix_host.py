"""CPU: the float64 reference of action-prefix conditioning (tests/flow_prefix_util.py) held to facts of its own, the host side of the feature
(fastvla_hip/prefix.py: the delay table, the widening, the checks that run before any engine exists, the checkpoint record), and the torch reference of the
bimodal toy whose fractions the GPU test is held to."""
import math

import numpy as np
import pytest
import torch

import flow_prefix_util as pu
import flow_util as fu
from fastvla_hip import prefix


# ------------------------------------------------------------------------------------------------------------------ noising
def test_prefix_noising_copies_the_prefix_and_keeps_the_rest():
    K, A, B = 5, 3, 7
    g = torch.Generator().manual_seed(1)
    a, eps, t = torch.randn(B, K * A, generator=g).numpy(), torch.randn(B, K * A, generator=g).numpy(), torch.rand(B, generator=g).numpy()
    delays = np.array([0, 1, 4, 2, 0, 3, 4])
    x, u = pu.prefix_noising_ref(a, eps, t, delays, K)
    x0, u0 = fu.noising_ref(a, eps, t)
    for r, d in enumerate(delays):
        assert np.array_equal(x[r, :d * A], a[r, :d * A].astype(np.float64)) and np.array_equal(x[r, d * A:], x0[r, d * A:])
    assert np.array_equal(u, u0)                                          # the mask removes the prefix from the loss, not the target
    m = pu.mask_ref(delays, K)
    assert set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(m.sum(axis=1), delays)


# ------------------------------------------------------------------------------------------------------------------ the delay table and its draw
@pytest.mark.parametrize("D,dist,rate", [(1, "uniform", 0.0), (2, "uniform", 0.0), (12, "uniform", 0.0), (12, "exp", 0.3), (49, "exp", 0.1), (1, "exp", 2.0)])
def test_delay_draw_reproduces_the_table(D, dist, rate):
    thr = prefix.delay_thresholds(D, dist, rate)
    assert len(thr) == D + 1 and thr[-1] == 1 << 24 and all(b >= a for a, b in zip(thr, thr[1:])) and thr[0] >= 0
    p_want = prefix.delay_probabilities(D, dist, rate)
    p_tab = prefix.table_probabilities(thr)
    assert abs(sum(p_tab) - 1.0) < 1e-12 and max(abs(a - b) for a, b in zip(p_tab, p_want)) <= 2.0 ** -24
    if dist == "exp" and D > 1:
        assert all(math.isclose(p_want[d + 1] / p_want[d], math.exp(-rate), rel_tol=1e-12) for d in range(D))
    n = 1 << 16
    d = pu.draw_delays(n, 0xC0FFEE, 5, thr)
    assert d.min() >= 0 and d.max() <= D
    counts = np.bincount(d, minlength=D + 1)
    for j in range(D + 1):                                                  # within 4 sigma of the binomial
        sigma = math.sqrt(n * p_tab[j] * (1.0 - p_tab[j]))
        assert abs(counts[j] - n * p_tab[j]) <= 4.0 * sigma + 1e-9, (j, counts[j], n * p_tab[j], sigma)
    assert np.array_equal(pu.draw_delays(5, 0xC0FFEE, 5, thr), d[:5])       # a row's delay does not depend on the batch
    assert not np.array_equal(pu.draw_delays(n, 0xC0FFEE, 6, thr), d)


def test_delay_table_refuses_bad_input():
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError):
            prefix.delay_thresholds(bad)
    with pytest.raises(ValueError):
        prefix.delay_thresholds(3, "gauss")
    with pytest.raises(ValueError):
        prefix.delay_thresholds(3, "exp", -1.0)
    K = 3
    assert prefix.delay_thresholds(K - 1)[-1] == 1 << 24                    # D = K - 1 works


# ------------------------------------------------------------------------------------------------------------------ the sampler reference
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_prefix_sampler_reference_reduces_to_the_plain_one_and_pins_exactly(name):
    B, N = 9, 4
    c = pu.prefix_case(name, B)
    K, A, E, D = c["dims"][4], c["dims"][5], c["dims"][6], c["D"]
    zero = np.zeros(B, dtype=np.int32)
    act, chunk = pu.prefix_euler_sample(c["p"], c["pooled"], c["states"], c["noise"], c["prev"], zero, 0, N, E, K, D)
    plain = fu.euler_sample(pu.drop_mask_columns(c["p"], K), c["pooled"], c["states"], c["noise"], N, E)
    assert torch.equal(act, chunk) and float((chunk - plain).abs().max()) <= 1e-12 * float(plain.abs().max())
    for shift in pu.SHIFTS(K) + (K,):
        _, chunk = pu.prefix_euler_sample(c["p"], c["pooled"], c["states"], c["noise"], c["prev"], c["delays"], shift, N, E, K, D)
        pin = pu.pinned_steps(c["delays"], D, K, shift)
        assert int(pin.max()) <= min(D, K - shift)
        for b in range(B):
            n = int(pin[b]) * A
            assert torch.equal(chunk[b, :n], c["prev"][b, shift * A:shift * A + n].double())
            assert not torch.equal(chunk[b, n:], c["noise"][b, n:].double())


@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_fp32_emulation_stays_within_1e_4_of_float64(name, B):
    """every case tests/test_gpu_flow_prefix.py runs: the bar tests/test_flow_host.py sets for the plain sampler"""
    K = fu.DIMS[name][4]
    worst = 0.0
    for shift in pu.SHIFTS(K):
        for io in (False, True):
            for N in fu.SAMPLER_STEPS:
                _, _, ea, ec = pu.prefix_refs(name, B, N, io, shift)
                worst = max(worst, ea, ec)
                assert 0.0 < ea <= 1e-4 and 0.0 < ec <= 1e-4, (name, B, shift, io, N, ea, ec)
    print(f"[prefix emulation {name} B={B}] worst distance from float64 {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------ widening
def test_widened_flow_head_computes_the_plain_velocity_for_m_zero():
    feat, ds, hid, fus, K, A, E = fu.DIMS["awkward"]
    da, B = K * A, 5
    p = fu.flow_head_params(fu.flow_head_shapes(feat, ds, da, hid, fus, E), 3)
    wide = prefix.widen_flow_state_dict(p, K)
    assert wide["fusion.0.weight"].shape == (fus, feat + hid + da + E + K) and bool((wide["fusion.0.weight"][:, -K:] == 0).all())
    assert torch.equal(wide["fusion.0.weight"][:, :-K], p["fusion.0.weight"]) and p["fusion.0.weight"].shape[1] == feat + hid + da + E      # a copy
    assert all(wide[k] is p[k] for k in p if k != "fusion.0.weight")
    g = torch.Generator().manual_seed(2)
    pooled, states, x = torch.randn(B, feat, generator=g).double(), torch.randn(B, ds, generator=g).double(), torch.randn(B, da, generator=g).double()
    phi = fu.phi_exact(np.full(B, 0.3), E)
    p64, w64 = {k: v.double() for k, v in p.items()}, {k: v.double() for k, v in wide.items()}
    assert torch.equal(pu.velocity(w64, pooled, states, x, phi, torch.zeros(B, K, dtype=torch.float64)), fu.velocity(p64, pooled, states, x, phi))
    # prefixed names (a policy's state dict) are found by suffix; an ambiguous or missing key is refused
    named = prefix.widen_flow_state_dict({"model." + k: v for k, v in p.items()}, K)
    assert named["model.fusion.0.weight"].shape[1] == feat + hid + da + E + K
    with pytest.raises(ValueError):
        prefix.widen_flow_state_dict({"a": torch.zeros(1)}, K)
    with pytest.raises(ValueError):
        prefix.widen_flow_state_dict(p, 1)


# ------------------------------------------------------------------------------------------------------------------ errors before any engine exists
def test_every_refusal_is_a_value_error_before_any_engine(monkeypatch):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy, resolve_prefix_options, resolve_rtc_options
    from vla_fastvlm.model import fastvlm_adapter
    for k in ("FASTVLA_FLOW_PREFIX_MAX_DELAY", "FASTVLA_FLOW_PREFIX_DELAY_DIST", "FASTVLA_FLOW_PREFIX_DELAY_RATE", "FASTVLA_RTC", "FASTVLA_RTC_METHOD",
              "FASTVLA_ACTION_HEAD", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "FASTVLA_CHUNK_SIZE", "FASTVLA_N_ACTION_STEPS"):
        monkeypatch.delenv(k, raising=False)

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(fastvlm_adapter.FastVLMBackbone, "engine", no_engine)
    cfg = FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0)
    cases = [(dict(chunk_size=8, action_head="regression", flow_prefix_max_delay=3), ("flow_prefix_max_delay", "action_head")),
             (dict(chunk_size=1, action_head="flow", flow_prefix_max_delay=1), ("flow_prefix_max_delay", "chunk_size")),
             (dict(chunk_size=8, action_head="flow", flow_prefix_max_delay=8), ("flow_prefix_max_delay", "chunk_size")),
             (dict(chunk_size=8, n_action_steps=1, action_head="flow", flow_prefix_max_delay=3, temporal_ensemble_coeff=0.01), ("flow_prefix_max_delay", "temporal_ensemble_coeff")),
             (dict(chunk_size=8, action_head="flow", flow_prefix_max_delay=0), ("flow_prefix_max_delay",)),
             (dict(chunk_size=8, action_head="flow", flow_prefix_max_delay=3, flow_prefix_delay_dist="gauss"), ("flow_prefix_delay_dist",)),
             (dict(chunk_size=8, n_action_steps=3, action_head="flow", rtc=True, rtc_method="prefix"), ("rtc_method", "flow_prefix_max_delay")),
             (dict(chunk_size=8, n_action_steps=3, action_head="flow", flow_prefix_max_delay=3, rtc=True, rtc_method="prefix", rtc_schedule="exp"), ("rtc_schedule", "prefix")),
             (dict(chunk_size=8, n_action_steps=3, action_head="flow", flow_prefix_max_delay=3, rtc=True, rtc_method="prefix", rtc_max_guidance_weight=2.0),
              ("rtc_max_guidance_weight", "prefix")),
             (dict(chunk_size=8, n_action_steps=3, action_head="flow", flow_prefix_max_delay=3, rtc=True, rtc_method="prefix", rtc_execution_horizon=2),
              ("rtc_execution_horizon", "prefix")),
             (dict(chunk_size=8, n_action_steps=3, action_head="flow", flow_prefix_max_delay=3, rtc=True, rtc_method="prefix", rtc_prefix_steps=4),
              ("rtc_prefix_steps", "flow_prefix_max_delay")),
             (dict(chunk_size=8, n_action_steps=3, action_head="flow", flow_prefix_max_delay=3, rtc=True, rtc_method="jacobian"), ("rtc_method",))]
    for kw, words in cases:
        with pytest.raises(ValueError) as e:
            FastVLAPolicy(cfg, **kw)
        assert all(w in str(e.value) for w in words), (kw, str(e.value))
    # the resolved records, and the environment twins (read for a flow head only)
    rec = resolve_prefix_options(3, "exp", 0.25, action_head="flow", chunk_size=8)
    assert rec == {"chunk": 8, "max_delay": 3, "dist": "exp", "rate": 0.25, "thresholds": prefix.delay_thresholds(3, "exp", 0.25)}
    assert resolve_prefix_options(action_head="flow", chunk_size=8) is None
    assert resolve_rtc_options(True, action_head="flow", chunk_size=8, n_action_steps=3, rtc_method="prefix", prefix=rec) == {"method": "prefix", "prefix_steps": 3, "max_delay": 3}
    assert resolve_rtc_options(True, action_head="flow", chunk_size=8, n_action_steps=3, rtc_method="prefix", rtc_prefix_steps=1, prefix=rec)["prefix_steps"] == 1
    assert "method" not in resolve_rtc_options(True, action_head="flow", chunk_size=8, n_action_steps=3, prefix=rec)      # the default stays guidance, on either width
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_MAX_DELAY", "2")
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_DELAY_DIST", "exp")
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_DELAY_RATE", "0.75")
    assert resolve_prefix_options(action_head="regression", chunk_size=8) is None
    got = resolve_prefix_options(action_head="flow", chunk_size=8)
    assert (got["max_delay"], got["dist"], got["rate"]) == (2, "exp", 0.75)
    assert resolve_prefix_options(False, action_head="flow", chunk_size=8) is None
    assert resolve_prefix_options(5, action_head="flow", chunk_size=8)["max_delay"] == 5                     # an explicit argument beats its twin
    monkeypatch.setenv("FASTVLA_RTC_METHOD", "prefix")
    assert resolve_rtc_options(True, action_head="flow", chunk_size=8, n_action_steps=3, prefix=got)["method"] == "prefix"
    with pytest.raises(ValueError, match="inference_delay"):
        prefix.check_inference_delay(4, 3)
    assert prefix.check_inference_delay(3, 3) == 3


# ------------------------------------------------------------------------------------------------------------------ the record and the module tree
def test_policy_modules_record_and_checkpoint_round_trip(monkeypatch, tmp_path):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy
    from vla_fastvlm.utils.checkpoint import check_fusion_width, flow_kwargs, prefix_kwargs
    for k in ("FASTVLA_FLOW_PREFIX_MAX_DELAY", "FASTVLA_RTC", "FASTVLA_ACTION_HEAD", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "FASTVLA_CHUNK_SIZE"):
        monkeypatch.delenv(k, raising=False)
    cfg = FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0)
    K, A, E, D = 3, cfg.action_dim, 6, 2
    kw = dict(chunk_size=K, action_head="flow", flow_steps=4, flow_time_dim=E, flow_seed=9)
    plain, pre = FastVLAPolicy(cfg, **kw), FastVLAPolicy(cfg, flow_prefix_max_delay=D, flow_prefix_delay_dist="exp", flow_prefix_delay_rate=0.25, **kw)
    assert pre.model.fusion[0].in_features == plain.model.fusion[0].in_features + K and list(pre.state_dict()) == list(plain.state_dict())
    rec = pre.model.flow_record()
    assert {k: rec[k] for k in ("prefix_max_delay", "prefix_delay_dist", "prefix_delay_rate")} == {"prefix_max_delay": D, "prefix_delay_dist": "exp", "prefix_delay_rate": 0.25}
    assert "prefix_max_delay" not in plain.model.flow_record()                 # a plain flow head's record is what it was
    # the record round-trips through the loader's keyword builders and through the extras helpers
    again = FastVLAPolicy(cfg, chunk_size=K, **flow_kwargs(rec), **prefix_kwargs(rec))
    assert again.flow_prefix == pre.flow_prefix and again.model.flow_record() == rec
    assert prefix_kwargs(plain.model.flow_record()) == {"flow_prefix_max_delay": False} and prefix_kwargs(None) == {"flow_prefix_max_delay": False}
    assert prefix.extras_record(None) == {}
    monkeypatch.setenv("FASTVLA_FLOW_PREFIX_MAX_DELAY", "1")                      # the file decides, whatever the twin says
    assert FastVLAPolicy(cfg, chunk_size=K, **flow_kwargs(plain.model.flow_record()), **prefix_kwargs(plain.model.flow_record())).flow_prefix is None
    monkeypatch.delenv("FASTVLA_FLOW_PREFIX_MAX_DELAY")
    # a checkpoint of the other width fails, naming fusion.0.weight's two shapes
    for pol, other in ((pre, plain), (plain, pre)):
        with pytest.raises(ValueError) as e:
            check_fusion_width({"model.fusion.0.weight": other.model.fusion[0].weight.detach()}, pol, "ckpt")
        assert str(tuple(other.model.fusion[0].weight.shape)) in str(e.value) and str(tuple(pol.model.fusion[0].weight.shape)) in str(e.value)
        assert "fusion.0.weight" in str(e.value) and "flow_prefix_max_delay" in str(e.value)
    # ... and loads after widening
    wide = prefix.widen_flow_state_dict(plain.state_dict(), K)
    check_fusion_width(wide, pre, "ckpt")
    pre.load_state_dict(wide)
    assert torch.equal(pre.model.fusion[0].weight[:, :-K], plain.model.fusion[0].weight) and bool((pre.model.fusion[0].weight[:, -K:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ the toy's torch reference
def test_bimodal_toy_reference_pins_the_mode():
    """the recipe the GPU test runs on the project's kernels (flow_prefix_util.PREFIX_BIMODAL), here on torch: pinning the first step to a + chunk's puts the
    other three steps in the + mode; unpinned samples land in both modes"""
    res = pu.prefix_bimodal_reference()
    print(f"[prefix bimodal reference] {res}")
    assert res["pinned"]["plus"] >= 0.9 and res["pinned"]["mean_abs"] >= 0.7
    assert res["pinned"]["plus"] >= 1.0                                           # the figure the GPU test's bar is derived from (its PINNED_REFERENCE)
    assert res["free"]["plus"] >= 0.35 and res["free"]["minus"] >= 0.35 and res["free"]["mean_abs"] >= 0.7
