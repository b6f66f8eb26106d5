"""Host-side checks of flow_noise_draws (no GPU): option resolution and its errors, the draw-offset rule against the host's offset layout, and the float64
multi-draw reference of tests/flow_draws_util.py against the mean of single-draw references."""
import numpy as np
import pytest
import torch

import flow_draws_util as du
import flow_util as fu
from chunk_loss_util import ragged_pad

FLOW_ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_STEPS", "FASTVLA_FLOW_TIME_DIM", "FASTVLA_FLOW_TIME_DIST", "FASTVLA_FLOW_NOISE_DRAWS")


def test_option_resolution_and_every_value_error(monkeypatch):
    from vla_fastvlm.fastvla.modeling_fastvla import resolve_flow_noise_draws as res
    for k in FLOW_ENV:
        monkeypatch.delenv(k, raising=False)
    assert res(None, action_head="flow") == 1 and res(None, action_head="regression") == 1
    assert res(5, action_head="flow") == 5 and res(16, action_head="flow") == 16 and res(1, action_head="regression") == 1
    monkeypatch.setenv("FASTVLA_FLOW_NOISE_DRAWS", "4")
    assert res(None, action_head="flow") == 4
    assert res(2, action_head="flow") == 2                                # the argument beats the twin
    assert res(None, action_head="regression") == 1                       # the twin is read for a flow head only
    for raw in ("0", "17", "-3", "2.5", "many"):
        monkeypatch.setenv("FASTVLA_FLOW_NOISE_DRAWS", raw)
        assert res(None, action_head="regression") == 1                   # ... and checked for a flow head only
        with pytest.raises(ValueError, match="FASTVLA_FLOW_NOISE_DRAWS"):
            res(None, action_head="flow")
    monkeypatch.delenv("FASTVLA_FLOW_NOISE_DRAWS")
    for bad in (0, 17, -1, 2.5, "3", True, [2]):
        with pytest.raises(ValueError) as ei:
            res(bad, action_head="flow")
        assert "flow_noise_draws" in str(ei.value) and "action_head" in str(ei.value)
    with pytest.raises(ValueError) as ei:                                  # an explicit S > 1 with the regression head names both settings
        res(3, action_head="regression")
    assert "flow_noise_draws=3" in str(ei.value) and "action_head='regression'" in str(ei.value)


def test_policies_take_the_option_before_any_engine_exists(monkeypatch):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    for k in FLOW_ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0)
    flow = FastVLAPolicy(cfg, chunk_size=3, action_head="flow", flow_time_dim=6, flow_noise_draws=4)
    assert flow.flow_noise_draws == 4 and flow.model.flow_noise_draws == 4 and flow.model.backbone.head_spec.draws == 4
    assert flow.model.backbone._engine is None                             # nothing was built
    assert "draws" not in flow.model.flow_record() and "noise_draws" not in flow.model.flow_record()      # a property of the run: no checkpoint key
    plain = FastVLAPolicy(cfg, chunk_size=3, action_head="flow", flow_time_dim=6)
    assert plain.flow_noise_draws == 1 and plain.model.backbone.head_spec.draws == 1
    assert list(plain.state_dict()) == list(flow.state_dict())
    for kw in (dict(flow_noise_draws=2), dict(action_head="regression", flow_noise_draws=8)):
        with pytest.raises(ValueError, match="action_head"):
            FastVLAPolicy(cfg, chunk_size=3, **kw)
    for bad in (0, 17, 1.5):
        with pytest.raises(ValueError, match="flow_noise_draws"):
            FastVLAPolicy(cfg, chunk_size=3, action_head="flow", flow_noise_draws=bad)
    monkeypatch.setenv("FASTVLA_FLOW_NOISE_DRAWS", "6")
    assert FastVLAPolicy(cfg, chunk_size=3, action_head="flow", flow_time_dim=6).flow_noise_draws == 6
    assert FastVLAPolicy(cfg, chunk_size=3).flow_noise_draws == 1         # regression head: the twin is ignored
    monkeypatch.setenv("FASTVLA_FLOW_NOISE_DRAWS", "99")
    assert FastVLAPolicy(cfg, chunk_size=3).flow_noise_draws == 1
    with pytest.raises(ValueError):
        FastVLAPolicy(cfg, chunk_size=3, action_head="flow")


def test_draw_offsets_do_not_collide_with_the_host_layout():
    from fastvla_hip.engine import FLOW_DRAWS_MAX, flow_draw_offset
    from vla_fastvlm.fastvla.fastvlm_with_expert import FastVLMWithExpert
    S = 16
    assert FLOW_DRAWS_MAX == S
    top = FastVLMWithExpert.flow_train_offset(4095, (1 << 28) - 1, 0xFFFF)      # the largest train offset: every bit below 56
    assert top == (1 << 56) - 1 and top == du.train_offset(4095, (1 << 28) - 1, 0xFFFF)
    with pytest.raises(ValueError, match="4096"):
        FastVLMWithExpert.flow_train_offset(4096, 0, 1)
    bases = [0, 1, top, FastVLMWithExpert.flow_train_offset(7, 123456, 3), (1 << 60) + 5, (1 << 61) + 9, (1 << 62) + 2]
    seen = {}
    for o in bases:
        for s in range(S):
            d = flow_draw_offset(o, s)
            assert d == o + (s << 56) and d < (1 << 63)
            assert d & ((1 << 56) - 1) == o & ((1 << 56) - 1)              # rank / step / micro stay what they were
            assert d >> 60 == o >> 60                                      # ... and so does the range marker
            assert (d >> 56) & 15 == s
            assert seen.setdefault(d, (o, s)) == (o, s)                    # no two (step, draw) pairs share an offset
    assert flow_draw_offset(top, 0) == top                                  # draw 0 is the single draw
    for bad_o in (1 << 56, 5 << 57, top + 1):
        with pytest.raises(ValueError):
            flow_draw_offset(bad_o, 1)
    for bad_s in (-1, 16):
        with pytest.raises(ValueError):
            flow_draw_offset(0, bad_s)


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("B,S", [(1, 2), (3, 5), (2, 8)])
def test_multi_draw_reference_is_the_mean_of_single_draw_references(B, S, kind):
    """in the reference's own float64 arithmetic: loss and the 12 gradients equal the mean over draws, d_pooled the SUM over draws of each single-draw
    d_pooled divided by S (every single-draw loss divides by B K A, the S-draw loss by S B K A).  The identity is exact in real arithmetic; the two sides
    add the same float64 terms in another order (a product over S B rows against S products over B rows), which moves a sum of n terms by at most n 2^-53
    relative to the sum of their magnitudes: with n <= a few hundred here the bar is 1e-12 of the value (and 1e-14 absolute for gradients that are 0)"""
    name = "awkward"
    c = du.case(name, B, S)
    K, A = c["dims"][4], c["dims"][5]
    pad = ragged_pad(B, K, seed=2) if B > 1 else None
    g = torch.Generator().manual_seed(3)
    dim_w, step_w = (torch.rand(A, generator=g) * 2, torch.rand(K, generator=g) * 2) if kind == "l1" else (None, None)
    args = (c["p"], c["pooled"], c["states"], c["a"], c["eps"], c["t"], pad, kind, S, c["dims"], dim_w, step_w)
    multi, mean = du.draws_reference(*args), du.mean_of_singles(*args)
    tol = dict(rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(float(multi["loss"]), float(mean["loss"]), **tol)
    for k, gk in multi["grads"].items():
        np.testing.assert_allclose(gk.numpy(), mean["grads"][k].numpy(), err_msg=k, **tol)
    np.testing.assert_allclose(multi["d_pooled"].numpy(), (sum(mean["d_pooled_each"]) / S).numpy(), **tol)
    assert multi["d_pooled"].shape == c["pooled"].shape and multi["pred"].shape == (S * B, K * A)
    # draw 0 of the S-draw reference is the single-draw reference's prediction
    one = du.draws_reference(*args, rows=[0])
    np.testing.assert_allclose(multi["pred"][:B].numpy(), one["pred"].numpy(), **tol)
    assert float(multi["grads"]["fusion.0.weight"].abs().max()) > 0 and float(multi["d_pooled"].abs().max()) > 0


def test_check_flow_draws():
    from fastvla_hip.engine import check_flow_draws
    assert [check_flow_draws(s) for s in (1, 2, 16, 4.0)] == [1, 2, 16, 4]
    for bad in (0, 17, -2, 1.5, "2", None, True):
        with pytest.raises(ValueError):
            check_flow_draws(bad)


def test_lerobot_plugin_takes_the_same_argument_and_twin(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    for k in FLOW_ENV:
        monkeypatch.delenv(k, raising=False)
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}

    def cfg():
        return LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=4, n_action_steps=2,
                        output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(5,))}, dropout=0.0)

    fields = set(vars(cfg()))
    pol = LRPolicy(cfg(), action_head="flow", flow_time_dim=6, flow_noise_draws=3)
    assert pol.flow_noise_draws == 3 and pol.model.flow_noise_draws == 3 and pol.model.backbone.head_spec.draws == 3 and pol.model.backbone._engine is None
    assert set(vars(pol.config)) == fields                                 # the registered config gains no field
    assert LRPolicy(cfg(), action_head="flow", flow_time_dim=6).flow_noise_draws == 1
    with pytest.raises(ValueError, match="action_head"):
        LRPolicy(cfg(), flow_noise_draws=3)
    with pytest.raises(ValueError, match="flow_noise_draws"):
        LRPolicy(cfg(), action_head="flow", flow_noise_draws=17)
    monkeypatch.setenv("FASTVLA_FLOW_NOISE_DRAWS", "5")
    assert LRPolicy(cfg(), action_head="flow", flow_time_dim=6).flow_noise_draws == 5
    assert LRPolicy(cfg()).flow_noise_draws == 1                          # regression head: the twin is ignored
