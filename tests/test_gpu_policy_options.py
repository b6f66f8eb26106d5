"""GPU: every option of tests/test_policy_options_host.py's "everything" row, on both policy surfaces -- the engine a backbone builds carries what the
HeadSpec says, a rebuilt engine (load_backbone_state) carries it again, and two policies built alike stay alike bit for bit, before and after the rebuild.
synthetic:tiny, state 6, action 5, K = 3, B = 1 and 2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402

K, A, DS = 3, 5, 6
EVERYTHING = dict(action_head="flow", flow_steps=2, flow_time_dim=6, flow_seed=21, flow_noise_draws=2, flow_prefix_max_delay=1, rtc=True, rtc_method="prefix",
                  flow_solver="heun", flow_samples=3, flow_select="coherent", action_dim_weights=[1.0, 1.0, 1.0, 1.0, 4.0], action_step_weights=[1.0, 0.5, 0.25])


@pytest.fixture(autouse=True)
def _twins(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("FASTVLA_") and k.split("_")[1] in ("ACTION", "FLOW", "RTC", "CHUNK", "N", "TEMPORAL")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("FASTVLA_ACTION_LOSS", "smooth_l1")      # (the LeRobot surface takes the loss kind from its twins only)
    monkeypatch.setenv("FASTVLA_ACTION_LOSS_BETA", "0.5")


def _mirrors_equal_the_spec(pol):
    bb = pol.model.backbone
    eng, spec = bb.engine(), bb.head_spec
    assert spec.flow is not None and spec.prefix is not None and spec.loss == dict(kind="smooth_l1", beta=0.5, chunk=K) and spec.solver_rows
    assert eng.head_flow == spec.flow and eng.head_flow_prefix == spec.prefix and eng.head_flow_draws == spec.draws == 2
    assert eng.head_flow_samples == dict(max_samples=3, weights=spec.samples["step_weights"]) and spec.samples["max_samples"] == 3
    assert eng.head_flow_solver == spec.solver == "heun" and eng.head_flow_solver_rows
    assert eng.head_flow_guidance is None and spec.guidance is None      # (rtc_method="prefix": no guidance to configure)
    assert eng.head_loss == spec.loss and eng.head_loss_weights == spec.loss_weights == {"dim": EVERYTHING["action_dim_weights"], "step": EVERYTHING["action_step_weights"]}
    return eng


def _rebuild(pol):
    bb = pol.model.backbone
    old = bb.engine()
    bb.load_backbone_state(dict(bb.source_tensors()))      # (the same tensors: the engine is closed and built again on the next use)
    assert bb._engine is None and _mirrors_equal_the_spec(pol) is not old


def test_core_surface():
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy

    def build():
        torch.manual_seed(5)
        return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", state_dim=DS, action_dim=A, hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K,
                             n_action_steps=2, **EVERYTHING).to(DEV)

    a, b = build(), build()
    g = torch.Generator().manual_seed(6)
    batch = {"images": torch.rand(2, 3, 72, 96, generator=g).to(DEV), "states": torch.randn(2, DS, generator=g).to(DEV), "actions": torch.randn(2, K, A, generator=g).to(DEV),
             "action_is_pad": torch.tensor([[False, False, True], [False, False, False]]), "tasks": ["stack the red block", "open drawer"]}
    img, st, task = batch["images"][0], batch["states"][0], "open drawer"
    for rebuilt in (False, True):
        for pol in (a, b):
            _rebuild(pol) if rebuilt else _mirrors_equal_the_spec(pol)
        first, second = (tuple(pol.select_action_chunk(img, st, task, DEV) for _ in range(2)) for pol in (a, b))      # (the second plan continues the first)
        assert first[0].shape == (K, A) and bool(torch.isfinite(first[0]).all()) and not torch.equal(first[0], first[1])
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
        assert a.last_candidates.shape == (1, 3, K, A) and torch.equal(a.last_choice, b.last_choice)
    for pol in (a, b):
        pol.train()
    la, lb = (float(pol.fused_train_step(batch, lr=1e-3)["loss"]) for pol in (a, b))
    assert la == lb and la > 0
    for pol in (a, b):
        pol.model.backbone.engine().close()


def test_lerobot_surface():
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(DS,))}

    def build():
        torch.manual_seed(5)
        cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, input_features=feats, chunk_size=K, n_action_steps=2,
                       output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
        return LRPolicy(cfg, **EVERYTHING).to(DEV)

    a, b = build(), build()
    g = torch.Generator().manual_seed(7)
    batch = {"observation.images.top": torch.rand(2, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(2, DS, generator=g).to(DEV), "task": ["a", "b"]}
    one = {k: v[:1] for k, v in batch.items()}
    for rebuilt, obs, B in ((False, one, 1), (True, batch, 2)):      # (the previous chunks are kept per environment of ONE engine: the rebuilt one starts over)
        for pol in (a, b):
            _rebuild(pol) if rebuilt else _mirrors_equal_the_spec(pol)
        first, second = (tuple(pol.predict_action_chunk(obs) for _ in range(2)) for pol in (a, b))      # (the second plan continues the first)
        assert first[0].shape == (B, K, A) and bool(torch.isfinite(first[0]).all()) and not torch.equal(first[0], first[1])
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
        assert a.last_candidates.shape == (B, 3, K, A) and torch.equal(a.last_choice, b.last_choice)
    train = {**batch, ACTION: torch.randn(2, K, A, generator=g).to(DEV), "action_is_pad": torch.tensor([[False, False, True], [False, False, False]])}
    for pol in (a, b):
        pol.train()
    (la, ia), (lb, ib) = (pol.forward(train) for pol in (a, b))
    assert float(la.detach()) == float(lb.detach()) and ia == ib and ia["loss"] > 0
    for pol in (a, b):
        pol.model.backbone.engine().close()
