"""CPU: real-time chunking's host side -- the prefix weights and the guidance weight against hand-computed values, the float64 guided reference held to
facts of its own (all-zero weights are the unguided sampler; the hard prefix converges on its target; the fp32 emulation stays close), and the ValueErrors
of prefix_weights and of the policy options, raised before any engine exists."""
import math

import numpy as np
import pytest
import torch

import flow_util as fu
import rtc_util as ru
from fastvla_hip.rtc import SCHEDULES, guidance_weight, prefix_weights


# ------------------------------------------------------------------------------------------------------------------ weights
def _e(c):
    return c * (math.e ** c - 1.0) / (math.e - 1.0)


# (K, d, s) -> schedule -> weights worked out by hand from the definition: c = (K - s - k) / (K - s - d + 1) on d <= k < K - s
HAND = {
    (8, 2, 3): {"exp": [1, 1, _e(3 / 4), _e(2 / 4), _e(1 / 4), 0, 0, 0], "linear": [1, 1, 0.75, 0.5, 0.25, 0, 0, 0],
                "ones": [1, 1, 1, 1, 1, 0, 0, 0], "zeros": [1, 1, 0, 0, 0, 0, 0, 0]},
    (5, 0, 1): {"exp": [_e(4 / 5), _e(3 / 5), _e(2 / 5), _e(1 / 5), 0], "linear": [0.8, 0.6, 0.4, 0.2, 0],
                "ones": [1, 1, 1, 1, 0], "zeros": [0, 0, 0, 0, 0]},
    (4, 3, 1): {"exp": [1, 1, 1, 0], "linear": [1, 1, 1, 0], "ones": [1, 1, 1, 0], "zeros": [1, 1, 1, 0]},
}


@pytest.mark.parametrize("kds", sorted(HAND))
def test_prefix_weights_match_hand_computed_values(kds):
    for schedule in SCHEDULES:
        got = prefix_weights(*kds, schedule)
        assert len(got) == kds[0] and all(isinstance(x, float) for x in got)
        np.testing.assert_allclose(got, HAND[kds][schedule], rtol=0, atol=1e-15, err_msg=f"{kds} {schedule}")
        np.testing.assert_allclose(ru.prefix_weights_ref(*kds, schedule), HAND[kds][schedule], rtol=0, atol=1e-15)
    # the exp values themselves, by hand: e^0.75 = 2.1170000, 0.75 * 1.1170000 / 1.7182818 = 0.4875510; e^0.5 = 1.6487213, 0.5 * 0.6487213 / 1.7182818 = 0.1887703
    assert abs(_e(0.75) - 0.4875510) < 1e-6 and abs(_e(0.5) - 0.1887703) < 1e-6


def test_guidance_weight_matches_the_formula():
    assert guidance_weight(1.0, 5.0) == 5.0 and guidance_weight(1.0, 0.25) == 0.25                 # t = 1: beta, no division by 0
    assert guidance_weight(0.5, 5.0) == 2.0                                                        # (0.25 + 0.25) / 0.25
    assert guidance_weight(0.5, 1.5) == 1.5
    assert abs(guidance_weight(0.25, 100.0) - (0.5625 + 0.0625) / 0.1875) < 1e-15
    t = float(np.float32(0.9))
    assert guidance_weight(t, 5.0) == 5.0 and abs(guidance_weight(t, 50.0) - ((1 - t) ** 2 + t * t) / ((1 - t) * t)) < 1e-12
    for N in (1, 4, 10):
        for ti in fu.step_times(N)[:-1]:
            assert guidance_weight(float(ti), 5.0) == ru.guidance_k(float(ti), 5.0) <= 5.0
    with pytest.raises(ValueError):
        guidance_weight(0.0, 5.0)


def test_prefix_weights_value_errors():
    for bad in ((0, 0, 1, "exp"), (4, -1, 1, "exp"), (4, 0, 0, "exp"), (4, 3, 2, "exp"), (4, 0, 5, "linear"), (4, 1.5, 1, "exp"), (4, 0, True, "exp"),
                (4, 0, 1, "cosine")):
        with pytest.raises(ValueError):
            prefix_weights(*bad)
    assert prefix_weights(4, 0, 4, "exp") == [0.0] * 4 and prefix_weights(4, 3, 1, "zeros") == [1.0, 1.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------ the reference, held to facts of its own
@pytest.mark.parametrize("name,B,N", [("awkward", 9, 4), ("larger", 1, 10), ("awkward", 1, 1)])
def test_all_zero_weights_are_the_unguided_sampler(name, B, N):
    case = ru.rtc_case(name, B)
    K, A, E = case["dims"][4], case["dims"][5], case["dims"][6]
    args = (case["p"], case["pooled"], case["states"], case["noise"], N, E)
    for io in (False, True):
        plain = fu.euler_sample(*args, **ru.io_kwargs(case, io))
        for Y, W in (ru.targets(case["prev"], np.zeros(K), K, A, 0), ru.targets(case["prev"], np.ones(K), K, A, K),
                     ru.targets(case["prev"], np.ones(K), K, A, 0, row_mask=np.zeros(B))):
            act, chunk = ru.guided_euler(*args, Y, W, ru.BETA, **ru.io_kwargs(case, io))
            assert torch.equal(act, plain)
            assert io or torch.equal(chunk, plain)


def test_targets_shift_and_select():
    prev = torch.arange(2 * 3 * 2, dtype=torch.float32).view(2, 6)
    prev[0, 0] = float("nan")
    Y, W = ru.targets(prev, [1.0, 0.5, 0.0], 3, 2, 1, row_mask=[1, 0])
    assert Y[0].tolist() == [2, 3, 4, 5, 0, 0] and W[0].tolist() == [1, 1, 0.5, 0.5, 0, 0] and W[1].abs().sum() == 0


def _third(K):
    return max(1, K // 3)


@pytest.mark.parametrize("N", [4, 10])
@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_hard_prefix_converges_and_fp32_emulation_stays_close(name, B, N):
    """d = s = K / 3 (at least one each), beta = 5, Y = the previous chunk itself: the guided sample's hard prefix ends within 0.1 x the distance at which
    the UNGUIDED sample of the same noise ends from the same Y; the fp32 emulation of the same run stays within 1e-4 of float64."""
    case = ru.rtc_case(name, B)
    K, A, E = case["dims"][4], case["dims"][5], case["dims"][6]
    d = s = _third(K)
    Y, W = ru.targets(case["prev"], ru.prefix_weights_ref(K, d, s, "exp"), K, A, 0)
    args = (case["p"], case["pooled"], case["states"], case["noise"], N, E)
    plain = fu.euler_sample(*args)
    _, chunk = ru.guided_euler(*args, Y, W, ru.BETA)
    _, chunk32 = ru.guided_euler(*args, Y, W, ru.BETA, fp32=True)
    got, free = ru.prefix_distance(chunk, Y, d, A), ru.prefix_distance(plain, Y, d, A)
    emu = fu.worst_row_vs_rms(chunk32, chunk)
    print(f"[rtc host {name} B={B} N={N}] hard prefix {got:.4f} vs unguided {free:.3f} (ratio {got / free:.4f}, bar 0.1); fp32 emulation {emu:.2e} (bar 1e-4)")
    assert got <= 0.1 * free
    assert emu <= 1e-4


# ------------------------------------------------------------------------------------------------------------------ the policy options, before any engine exists
def test_policy_option_value_errors(monkeypatch):
    from vla_fastvlm.fastvla.modeling_fastvla import resolve_rtc_options

    def opts(*a, head="flow", K=8, n=3, coeff=None):
        return resolve_rtc_options(*a, action_head=head, chunk_size=K, n_action_steps=n, temporal_ensemble_coeff=coeff)

    for k in ("FASTVLA_RTC", "FASTVLA_RTC_SCHEDULE", "FASTVLA_RTC_MAX_GUIDANCE_WEIGHT", "FASTVLA_RTC_EXECUTION_HORIZON"):
        monkeypatch.delenv(k, raising=False)
    assert opts() is None and opts(False) is None and opts(head="regression") is None
    assert opts(True) == {"schedule": "exp", "max_guidance_weight": 5.0, "execution_horizon": 3}
    assert opts(True, "linear", 2.5, 5) == {"schedule": "linear", "max_guidance_weight": 2.5, "execution_horizon": 5}
    with pytest.raises(ValueError, match=r"rtc=.*action_head="):
        opts(True, head="regression")
    with pytest.raises(ValueError, match=r"rtc=.*chunk_size=1"):
        opts(True, K=1, n=1)
    with pytest.raises(ValueError, match=r"rtc=.*temporal_ensemble_coeff="):
        opts(True, n=1, coeff=0.01)
    with pytest.raises(ValueError, match=r"rtc_execution_horizon=9.*chunk_size=8"):
        opts(True, None, None, 9)
    for bad in (dict(rtc_schedule="cosine"), dict(rtc_max_guidance_weight=0.0), dict(rtc_max_guidance_weight=float("nan")), dict(rtc_execution_horizon=0)):
        with pytest.raises(ValueError):
            resolve_rtc_options(True, **bad, action_head="flow", chunk_size=8, n_action_steps=3)
    # the twins, and the argument beating them
    monkeypatch.setenv("FASTVLA_RTC", "1")
    monkeypatch.setenv("FASTVLA_RTC_SCHEDULE", "ones")
    monkeypatch.setenv("FASTVLA_RTC_MAX_GUIDANCE_WEIGHT", "7.5")
    monkeypatch.setenv("FASTVLA_RTC_EXECUTION_HORIZON", "2")
    assert opts() == {"schedule": "ones", "max_guidance_weight": 7.5, "execution_horizon": 2}
    assert opts(None, "zeros") == {"schedule": "zeros", "max_guidance_weight": 7.5, "execution_horizon": 2} and opts(False) is None
    monkeypatch.setenv("FASTVLA_RTC", "0")
    assert opts() is None


def test_policy_constructor_raises_before_an_engine_exists(monkeypatch):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy
    for k in ("FASTVLA_RTC", "FASTVLA_ACTION_HEAD", "FASTVLA_CHUNK_SIZE"):
        monkeypatch.delenv(k, raising=False)
    cfg = FastVLAConfig(vlm_model_name="synthetic:tiny", state_dim=6, action_dim=7, hidden_dim=32, fusion_dim=48)
    with pytest.raises(ValueError, match="action_head"):
        FastVLAPolicy(cfg, chunk_size=8, n_action_steps=3, rtc=True)
    with pytest.raises(ValueError, match="chunk_size"):
        FastVLAPolicy(cfg, action_head="flow", flow_time_dim=6, rtc=True)
    with pytest.raises(ValueError, match="temporal_ensemble_coeff"):
        FastVLAPolicy(cfg, chunk_size=8, action_head="flow", flow_time_dim=6, temporal_ensemble_coeff=0.01, rtc=True)
    with pytest.raises(ValueError, match="chunk_size"):
        FastVLAPolicy(cfg, chunk_size=8, n_action_steps=3, action_head="flow", flow_time_dim=6, rtc=True, rtc_execution_horizon=9)
    pol = FastVLAPolicy(cfg, chunk_size=8, n_action_steps=3, action_head="flow", flow_time_dim=6, rtc=True)
    assert pol.rtc == {"schedule": "exp", "max_guidance_weight": 5.0, "execution_horizon": 3} and pol.model.backbone._engine is None
    assert pol.last_chunk_normalised is None
    with pytest.raises(ValueError, match="rtc"):
        FastVLAPolicy(cfg, chunk_size=8, action_head="flow", flow_time_dim=6).select_action_chunk(torch.zeros(3, 8, 8), torch.zeros(6), "t", "cpu",
                                                                                                  prev_chunk=torch.zeros(8, 7))
