"""CPU: the host side of action chunks -- the float64 reference of the chunked loss against torch, argument validation, state-dict shapes, the
hip_extras.json record and the core policy's action queue.  No device call is made."""
import json

import numpy as np
import pytest
import torch

from chunk_loss_util import KINDS, chunk_loss_ref, ragged_pad, torch_loss_ref
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
from vla_fastvlm.utils import load_policy_from_checkpoint
from vla_fastvlm.utils.checkpoint import EXTRAS_FILE, read_extras, save_policy_checkpoint


def _cfg(**kw):
    return FastVLAConfig(vlm_model_name="synthetic:tiny", hidden_dim=16, fusion_dim=16, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("masked", [False, True])
def test_reference_agrees_with_torch(kind, masked):
    g = torch.Generator().manual_seed(3)
    B, K, A, beta = 5, 4, 3, 0.7
    a = torch.randn(B, K, A, generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.randn(B, K, A, generator=g, dtype=torch.float64)
    with torch.no_grad():
        t[0, 0, 0] = a[0, 0, 0]                    # d == 0 exactly
        t[0, 0, 1] = a[0, 0, 1] - beta             # |d| == beta exactly (up to the subtraction's rounding: both sides of the branch agree there)
    pad = torch.from_numpy(ragged_pad(B, K)) if masked else None
    loss = torch_loss_ref(a, t, pad, kind, beta)
    loss.backward()
    ref = chunk_loss_ref(a.detach().numpy(), t.numpy(), None if pad is None else pad.numpy(), kind, beta, loss_scale=4.0)
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-14 * max(1.0, abs(float(loss.detach())))
    np.testing.assert_allclose(ref["g"], 4.0 * a.grad.numpy(), rtol=1e-13, atol=1e-16)
    mse = torch_loss_ref(a.detach(), t, pad, "mse")
    assert abs(ref["mse"] - float(mse)) <= 1e-14 and ref["valid"] == (1.0 if pad is None else float((~pad).double().mean()))


def test_reference_ignores_what_padded_targets_hold():
    a, t = np.ones((2, 2, 3)), np.zeros((2, 2, 3))
    pad = np.array([[False, True], [True, True]])
    t[0, 1], t[1, 0], t[1, 1] = np.nan, np.inf, -np.inf
    for kind in KINDS:
        r = chunk_loss_ref(a, t, pad, kind)
        assert np.isfinite(r["g"]).all() and r["valid"] == 0.25 and r["mse"] == 3.0 / 12.0
        assert (r["g"][pad] == 0).all() and (r["g"][~pad] != 0).all()


def test_argument_validation():
    with pytest.raises(ValueError, match="n_action_steps"):
        FastVLAPolicy(_cfg(), chunk_size=2, n_action_steps=3)
    with pytest.raises(ValueError, match="unknown action loss"):
        FastVLAPolicy(_cfg(), action_loss="huber")
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            FastVLAPolicy(_cfg(), action_loss="smooth_l1", action_loss_beta=beta)
    with pytest.raises(ValueError, match="chunk size"):
        FastVLAPolicy(_cfg(), chunk_size=0)
    pol = FastVLAPolicy(_cfg(), chunk_size=4, n_action_steps=2)
    A = pol.config.action_dim
    with pytest.raises(ValueError, match=rf"\(B, 4, {A}\)"):
        pol.model.chunk_targets(torch.zeros(3, A))                                   # (B, A) targets with K > 1
    with pytest.raises(ValueError, match=rf"\(B, 4, {A}\)"):
        pol.model.chunk_targets(torch.zeros(3, 3, A))
    with pytest.raises(ValueError, match="action_is_pad"):
        pol.model.chunk_targets(torch.zeros(3, 4, A), torch.zeros(3, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="action_is_pad"):
        pol.model.chunk_targets(torch.zeros(3, 4, A), torch.zeros(4, dtype=torch.bool))
    flat, pad = pol.model.chunk_targets(torch.arange(3 * 4 * A).view(3, 4, A).float(), torch.tensor(ragged_pad(3, 4)))
    assert flat.shape == (3, 4 * A) and flat[1, A] == 4 * A + A and pad.dtype == torch.bool and pad.shape == (3, 4)
    with pytest.raises(ValueError, match="unknown action loss"):
        pol.set_action_loss("l3")
    pol.set_action_loss("smooth_l1", 0.5)
    assert (pol.model.action_loss, pol.model.action_loss_beta) == ("smooth_l1", 0.5)
    # without chunks everything is accepted as before: (B, A), and step 0 of a longer (B, T, A)
    one = FastVLAPolicy(_cfg())
    t = torch.randn(3, 2, one.config.action_dim)
    assert torch.equal(one.model.chunk_targets(t)[0], t[:, 0]) and torch.equal(one.model.chunk_targets(t[:, 1])[0], t[:, 1])


def test_environment_twins(monkeypatch):
    monkeypatch.setenv("FASTVLA_CHUNK_SIZE", "6")
    monkeypatch.setenv("FASTVLA_N_ACTION_STEPS", "3")
    monkeypatch.setenv("FASTVLA_ACTION_LOSS", "smooth_l1")
    monkeypatch.setenv("FASTVLA_ACTION_LOSS_BETA", "0.25")
    pol = FastVLAPolicy(_cfg())
    assert (pol.chunk_size, pol.n_action_steps, pol.model.action_loss, pol.model.action_loss_beta) == (6, 3, "smooth_l1", 0.25)
    pol = FastVLAPolicy(_cfg(), chunk_size=2, n_action_steps=1, action_loss="l1")       # an explicit argument beats its twin
    assert (pol.chunk_size, pol.n_action_steps, pol.model.action_loss) == (2, 1, "l1")


def test_state_dict_shapes_with_four_steps():
    base, pol = FastVLAPolicy(_cfg()), FastVLAPolicy(_cfg(), chunk_size=4)
    A, fus = pol.config.action_dim, pol.config.fusion_dim
    sb, sp = base.state_dict(), pol.state_dict()
    assert list(sb) == list(sp)                                           # the keys are unchanged
    grown = {k for k in sb if sb[k].shape != sp[k].shape}
    assert grown == {"model.action_head.weight", "model.action_head.bias"}
    assert sp["model.action_head.weight"].shape == (4 * A, fus) and sp["model.action_head.bias"].shape == (4 * A,)
    assert pol.config == base.config and pol.model.backbone.head_spec.dims["action_dim"] == 4 * A
    # folded statistics stay A long in the state dict and are tiled over the steps only on their way to the kernels
    stats = dict(state_mean=torch.zeros(pol.config.state_dim), state_std=torch.ones(pol.config.state_dim), action_mean=torch.arange(A).float(),
                 action_std=torch.arange(A).float() + 1)
    pol.model.backbone.set_io_normalization(**stats)
    assert pol.state_dict()["model.backbone.io_norm.action_mean"].shape == (A,)
    tiled = pol.model.backbone._io_norm_for_engine()
    assert torch.equal(tiled["action_mean"], torch.arange(A).float().repeat(4)) and tiled["action_std"].shape == (4 * A,) and tiled["state_mean"].shape == (pol.config.state_dim,)


def test_extras_record_round_trip(tmp_path):
    pol = FastVLAPolicy(_cfg(), chunk_size=4, n_action_steps=3, action_loss="smooth_l1", action_loss_beta=0.5)
    d = save_policy_checkpoint(pol, tmp_path / "chunked")
    assert read_extras(d)["action_chunk"] == {"chunk_size": 4, "n_action_steps": 3, "loss": "smooth_l1", "beta": 0.5}
    again = load_policy_from_checkpoint(str(d))
    assert (again.chunk_size, again.n_action_steps, again.model.action_loss, again.model.action_loss_beta) == (4, 3, "smooth_l1", 0.5)
    for k, v in pol.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    # a loss other than MSE alone is recorded too (the head is A wide then)
    d = save_policy_checkpoint(FastVLAPolicy(_cfg(), action_loss="l1"), tmp_path / "l1")
    assert read_extras(d)["action_chunk"] == {"chunk_size": 1, "n_action_steps": 1, "loss": "l1", "beta": 1.0}
    assert load_policy_from_checkpoint(str(d)).model.action_loss == "l1"


def test_default_policy_writes_what_it_always_wrote(tmp_path):
    pol = FastVLAPolicy(_cfg())
    d = save_policy_checkpoint(pol, tmp_path / "plain")
    assert not (d / EXTRAS_FILE).exists()                                 # nothing differs from the defaults: no extras file at all
    pol.model.backbone.splice_image_tokens = True                         # ... and when another feature writes the file, it gains no key
    d = save_policy_checkpoint(pol, tmp_path / "splice")
    assert (d / EXTRAS_FILE).read_text() == json.dumps({"splice_image_tokens": True, "train_backbone": False, "train_tower": False}, indent=2)


def test_plain_checkpoint_loads_as_a_plain_policy_whatever_the_twins_say(tmp_path, monkeypatch):
    d = save_policy_checkpoint(FastVLAPolicy(_cfg()), tmp_path / "plain")
    monkeypatch.setenv("FASTVLA_N_ACTION_STEPS", "4")
    monkeypatch.setenv("FASTVLA_CHUNK_SIZE", "4")
    monkeypatch.setenv("FASTVLA_ACTION_LOSS", "l1")
    pol = load_policy_from_checkpoint(str(d))
    assert (pol.chunk_size, pol.n_action_steps, pol.model.action_loss, pol.model.action_loss_beta) == (1, 1, "mse", 1.0)


def test_chunk_targets_is_idempotent():
    pol = FastVLAPolicy(_cfg(), chunk_size=4)
    A = pol.config.action_dim
    t, pad = torch.randn(3, 4, A), torch.tensor(ragged_pad(3, 4))
    flat, p1 = pol.model.chunk_targets(t, pad)
    again, p2 = pol.model.chunk_targets(flat, p1)
    assert torch.equal(again, flat) and torch.equal(p2, p1)
    with pytest.raises(ValueError, match="action_is_pad"):
        pol.model.chunk_targets(flat, torch.zeros(3, 3, dtype=torch.bool))


def test_wide_head_without_a_record_raises(tmp_path):
    pol = FastVLAPolicy(_cfg(), chunk_size=4)
    d = save_policy_checkpoint(pol, tmp_path / "c")
    (d / EXTRAS_FILE).unlink()
    A, fus = pol.config.action_dim, pol.config.fusion_dim
    with pytest.raises(ValueError) as e:
        load_policy_from_checkpoint(str(d))
    assert f"({4 * A}, {fus})" in str(e.value) and f"({A}, {fus})" in str(e.value) and "action_chunk" in str(e.value)
    # ... and a record that disagrees with the tensors raises as well
    (d / EXTRAS_FILE).write_text(json.dumps({"action_chunk": {"chunk_size": 2, "n_action_steps": 1, "loss": "mse", "beta": 1.0}}))
    with pytest.raises(ValueError, match="chunk_size=2"):
        load_policy_from_checkpoint(str(d))


def test_select_action_queue_arithmetic():
    pol = FastVLAPolicy(_cfg(), chunk_size=4, n_action_steps=3)
    A, calls = pol.config.action_dim, []

    def counted_forward(images, states, tasks, device=None):
        calls.append(1)
        return (100.0 * len(calls) + torch.arange(4).float()).view(1, 4, 1).expand(1, 4, A).clone()     # row k of prediction p holds 100 p + k

    pol.forward = counted_forward
    img, st = torch.zeros(3, 8, 8), torch.zeros(pol.config.state_dim)
    got = [pol.select_action(img, st, "lift", torch.device("cpu")) for _ in range(7)]
    assert len(calls) == 3                                                # 7 calls at n = 3: predictions before calls 1, 4 and 7
    assert all(g.shape == (A,) for g in got)
    assert [float(g[0]) for g in got] == [100.0, 101.0, 102.0, 200.0, 201.0, 202.0, 300.0]      # rows 0, 1, 2 of each chunk in order; row 3 is never served
    pol.reset()                                                           # rows 1, 2 of the third chunk are dropped: the next call predicts
    assert float(pol.select_action(img, st, "lift", torch.device("cpu"))[0]) == 400.0 and len(calls) == 4
    chunk = pol.select_action_chunk(img, st, "lift", torch.device("cpu"))
    assert chunk.shape == (4, A) and len(calls) == 5 and float(chunk[3, 0]) == 503.0
    # n_action_steps = 1: a prediction on every call, step 0 served
    pol1 = FastVLAPolicy(_cfg(), chunk_size=4)
    n = []
    pol1.forward = lambda images, states, tasks, device=None: n.append(1) or torch.full((1, 4, A), float(len(n)))
    assert [float(pol1.select_action(img, st, "lift", torch.device("cpu"))[0]) for _ in range(3)] == [1.0, 2.0, 3.0]


def test_lerobot_wrapper_takes_chunk_size_from_its_config():
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import HAVE_LEROBOT, FeatureType, PolicyFeature
    if HAVE_LEROBOT:
        pytest.skip("stand-in semantics are only exercised without lerobot")
    feats = {"observation.images.top": PolicyFeature(FeatureType.VISUAL, (3, 96, 96)), "observation.state": PolicyFeature(FeatureType.STATE, (6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny", hidden_dim=16, fusion_dim=16, input_features=feats, chunk_size=4, n_action_steps=3,
                   output_features={"action": PolicyFeature(FeatureType.ACTION, (5,))})
    assert cfg.action_delta_indices == [0, 1, 2, 3]
    pol = LRPolicy(cfg)
    assert pol.model.chunk_size == 4 and pol.model.action_head.weight.shape == (20, 16)
    calls = []
    pol._predict_actions = lambda b: calls.append(1) or (10.0 * len(calls) + torch.arange(4).float()).view(1, 4, 1).expand(2, 4, 5).clone()
    got = [pol.select_action({}) for _ in range(7)]
    assert len(calls) == 3 and [float(g[0, 0]) for g in got] == [10.0, 11.0, 12.0, 20.0, 21.0, 22.0, 30.0] and got[0].shape == (2, 5)
