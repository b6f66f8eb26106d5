"""CPU: temporal ensembling's host side -- the two float64 references against each other, the derived fp32 error bar against an fp32 emulation, argument
validation, the environment twin, the hip_extras.json record and the select_action plumbing of both policy surfaces.  No device call is made."""
import json

import numpy as np
import pytest
import torch

from ensemble_util import ensemble_closed, ensemble_online, ensemble_online_fp32, error_bar, weights
from fastvla_hip.ensemble import check_coeff, reference_weights
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
from vla_fastvlm.fastvla.modeling_fastvla import parse_weight_list, resolve_chunk_options
from vla_fastvlm.utils import load_policy_from_checkpoint
from vla_fastvlm.utils.checkpoint import EXTRAS_FILE, read_extras, save_policy_checkpoint


def _cfg(**kw):
    return FastVLAConfig(vlm_model_name="synthetic:tiny", hidden_dim=16, fusion_dim=16, **kw)


@pytest.mark.parametrize("coeff", [0.01, 0.0, -0.5, 2.0])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 1), (3, 4, 5), (2, 7, 3)])
def test_online_and_closed_forms_agree(shape, coeff):
    n_env, K, A = shape
    T = 3 * K + 2
    chunks = np.random.default_rng(K * 10 + A).normal(0.0, 3.0, size=(T, n_env, K, A))
    resets = {K + 1: [0], 2 * K: [n_env - 1], 2 * K + 1: [None]}                  # one environment mid-run, another later, then all
    for rs in (None, resets):
        a, b = ensemble_online(chunks, coeff, rs), ensemble_closed(chunks, coeff, rs)
        assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(chunks).max()), (shape, coeff, rs)
    a = ensemble_online(chunks, coeff, resets)
    assert np.array_equal(a[0], chunks[0, :, 0])                                   # nothing to average yet: row 0 as it is
    assert np.array_equal(a[K + 1, 0], chunks[K + 1, 0, 0]) and np.array_equal(a[2 * K + 1], chunks[2 * K + 1, :, 0])      # ... and after a reset
    if K == 1:
        assert np.array_equal(a, chunks[:, :, 0])


def test_weights_are_act_s():
    w, cw = weights(0.01, 5)
    assert w[0] == 1.0 and np.all(np.diff(w) < 0) and cw[-1] == pytest.approx(w.sum())          # i = 0, the oldest, weighs most for coeff > 0
    rw, rcw = reference_weights(0.01, 5)
    assert np.array_equal(w, rw) and np.allclose(cw, rcw, rtol=1e-15)
    assert np.array_equal(weights(0.0, 4)[0], np.ones(4)) and weights(-0.5, 3)[0][2] > 1.0
    # uniform weights: the plain mean of what is there
    chunks = np.random.default_rng(0).normal(size=(4, 1, 3, 2))
    out = ensemble_closed(chunks, 0.0)
    assert np.allclose(out[2, 0], (chunks[0, 0, 2] + chunks[1, 0, 1] + chunks[2, 0, 0]) / 3.0, rtol=1e-15)


@pytest.mark.parametrize("K", [2, 4, 8, 50, 100])
def test_fp32_emulation_stays_below_a_quarter_of_the_derived_bar(K):
    rng = np.random.default_rng(K)
    for coeff in (0.01, 0.0, -0.5, 2.0):
        chunks = rng.normal(0.0, 3.0, size=(2 * K + 1, 2, K, 3)).astype(np.float32)
        ref, emu = ensemble_closed(chunks, coeff), ensemble_online_fp32(chunks, coeff)
        assert emu.dtype == np.float32
        worst = np.abs(emu.astype(np.float64) - ref).max() / error_bar(K, float(np.abs(chunks).max()))
        assert worst <= 0.25, (K, coeff, worst)


def test_argument_validation(monkeypatch):
    with pytest.raises(ValueError, match="n_action_steps.*temporal_ensemble_coeff|temporal_ensemble_coeff.*n_action_steps"):
        FastVLAPolicy(_cfg(), chunk_size=4, n_action_steps=2, temporal_ensemble_coeff=0.01)
    for bad in (float("nan"), float("inf"), float("-inf"), "x"):
        with pytest.raises(ValueError, match="finite"):
            FastVLAPolicy(_cfg(), chunk_size=4, temporal_ensemble_coeff=bad)
        with pytest.raises(ValueError):
            check_coeff(bad)
    assert FastVLAPolicy(_cfg(), chunk_size=4, temporal_ensemble_coeff=0).temporal_ensemble_coeff == 0.0        # 0 is a coefficient (uniform), not "off"
    assert FastVLAPolicy(_cfg(), chunk_size=4).temporal_ensemble_coeff is None
    monkeypatch.setenv("FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "0.25")
    assert FastVLAPolicy(_cfg(), chunk_size=4).temporal_ensemble_coeff == 0.25
    assert FastVLAPolicy(_cfg(), chunk_size=4, temporal_ensemble_coeff=-0.5).temporal_ensemble_coeff == -0.5    # an explicit argument beats the twin
    assert FastVLAPolicy(_cfg(), chunk_size=4, temporal_ensemble_coeff=False).temporal_ensemble_coeff is None   # ... also to switch it off
    monkeypatch.setenv("FASTVLA_N_ACTION_STEPS", "2")
    with pytest.raises(ValueError, match="n_action_steps"):
        FastVLAPolicy(_cfg(), chunk_size=4)
    monkeypatch.setenv("FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "nan")
    with pytest.raises(ValueError, match="finite"):
        FastVLAPolicy(_cfg(), chunk_size=4, n_action_steps=1)


def test_loss_weight_options(monkeypatch):
    A = _cfg().action_dim
    with pytest.raises(ValueError, match="action_dim_weights"):
        FastVLAPolicy(_cfg(), chunk_size=2, action_dim_weights=[1.0] * (A - 1))                  # wrong length
    with pytest.raises(ValueError, match="action_step_weights"):
        FastVLAPolicy(_cfg(), chunk_size=2, action_step_weights=[1.0, 1.0, 1.0])
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=">= 0"):
            FastVLAPolicy(_cfg(), chunk_size=2, action_step_weights=[1.0, bad])
    pol = FastVLAPolicy(_cfg(), chunk_size=3, action_step_weights="discount:0.5")
    assert pol.model.action_loss_weights == {"dim": None, "step": [1.0, 0.5, 0.25]}
    with pytest.raises(ValueError, match="action_dim_weights"):
        pol.set_action_loss_weights([1.0] * (A + 1))
    assert pol.model.action_loss_weights == {"dim": None, "step": [1.0, 0.5, 0.25]}              # a refused call changes nothing
    pol.set_action_loss_weights()
    assert pol.model.action_loss_weights is None
    monkeypatch.setenv("FASTVLA_ACTION_DIM_WEIGHTS", ",".join(["1"] * (A - 1) + ["4"]))
    monkeypatch.setenv("FASTVLA_ACTION_STEP_WEIGHTS", "discount:0.9")
    pol = FastVLAPolicy(_cfg(), chunk_size=2)
    assert pol.model.action_loss_weights == {"dim": [1.0] * (A - 1) + [4.0], "step": [1.0, 0.9]}
    monkeypatch.setenv("FASTVLA_ACTION_STEP_WEIGHTS", "2, 0")
    assert FastVLAPolicy(_cfg(), chunk_size=2, action_dim_weights=False).model.action_loss_weights == {"dim": None, "step": [2.0, 0.0]}
    assert parse_weight_list("1,2.5", "x") == [1.0, 2.5]
    with pytest.raises(ValueError, match="cannot read"):
        parse_weight_list("discount:0.9", "x")                                    # only the step weights know a discount
    with pytest.raises(ValueError, match="cannot read"):
        parse_weight_list("a,b", "x", 3)
    assert resolve_chunk_options(chunk_size=2)["step_weights"] == [2.0, 0.0]


def test_extras_record_round_trip(tmp_path, monkeypatch):
    A = _cfg().action_dim
    dim_w = [1.0] * (A - 1) + [4.0]
    pol = FastVLAPolicy(_cfg(), chunk_size=4, action_loss="l1", temporal_ensemble_coeff=0.01, action_dim_weights=dim_w, action_step_weights="discount:0.5")
    d = save_policy_checkpoint(pol, tmp_path / "ens")
    assert read_extras(d)["action_chunk"] == {"chunk_size": 4, "n_action_steps": 1, "loss": "l1", "beta": 1.0, "temporal_ensemble_coeff": 0.01,
                                              "dim_weights": dim_w, "step_weights": [1.0, 0.5, 0.25, 0.125]}
    again = load_policy_from_checkpoint(str(d))
    assert again.temporal_ensemble_coeff == 0.01 and again.model.action_loss_weights == {"dim": dim_w, "step": [1.0, 0.5, 0.25, 0.125]}
    # only what is set is written: a chunked policy's record is what it was
    d = save_policy_checkpoint(FastVLAPolicy(_cfg(), chunk_size=4, n_action_steps=3), tmp_path / "chunked")
    assert read_extras(d)["action_chunk"] == {"chunk_size": 4, "n_action_steps": 3, "loss": "mse", "beta": 1.0}
    d = save_policy_checkpoint(FastVLAPolicy(_cfg(), chunk_size=4, temporal_ensemble_coeff=0.0), tmp_path / "uniform")
    assert read_extras(d)["action_chunk"] == {"chunk_size": 4, "n_action_steps": 1, "loss": "mse", "beta": 1.0, "temporal_ensemble_coeff": 0.0}
    # the file decides: a record without the keys loads without them whatever the twins say
    monkeypatch.setenv("FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "0.5")
    monkeypatch.setenv("FASTVLA_ACTION_STEP_WEIGHTS", "discount:0.5")
    plain = load_policy_from_checkpoint(str(tmp_path / "chunked"))
    assert plain.temporal_ensemble_coeff is None and plain.model.action_loss_weights is None and plain.n_action_steps == 3


def test_default_policy_writes_what_it_always_wrote(tmp_path):
    pol = FastVLAPolicy(_cfg())
    d = save_policy_checkpoint(pol, tmp_path / "plain")
    assert not (d / EXTRAS_FILE).exists()
    pol.model.backbone.splice_image_tokens = True
    d = save_policy_checkpoint(pol, tmp_path / "splice")
    assert (d / EXTRAS_FILE).read_text() == json.dumps({"splice_image_tokens": True, "train_backbone": False, "train_tower": False}, indent=2)
    assert pol.model.chunk_record() is None and pol.model.action_loss_weights is None


class _FakeEnsembler:
    """stands in for fastvla_hip.TemporalEnsembler on the host: the float64 closed form over what step() has seen"""
    made = []

    def __init__(self, engine, n_env, chunk, step_dim, coeff):
        self._engine, self.n_env, self.coeff, self.seen, self._h = engine, n_env, coeff, [], 1
        _FakeEnsembler.made.append(self)

    def step(self, chunks):
        self.seen.append(chunks.double().numpy().reshape(self.n_env, chunks.shape[-2], chunks.shape[-1]))
        return torch.from_numpy(ensemble_closed(np.stack(self.seen), self.coeff)[-1])

    def close(self):
        self._h = None


def test_core_select_action_runs_the_backbone_every_step_and_ensembles(monkeypatch):
    import fastvla_hip.ensemble as ens_mod
    monkeypatch.setattr(ens_mod, "TemporalEnsembler", _FakeEnsembler)
    _FakeEnsembler.made.clear()
    pol = FastVLAPolicy(_cfg(), chunk_size=4, temporal_ensemble_coeff=0.0)
    A, calls = pol.config.action_dim, []
    monkeypatch.setattr(pol.model, "_engine", lambda: "engine")

    def counted_forward(images, states, tasks, device=None):
        calls.append(1)
        return (100.0 * len(calls) + torch.arange(4).float()).view(1, 4, 1).expand(1, 4, A).clone()     # row k of prediction p holds 100 p + k

    pol.forward = counted_forward
    img, st = torch.zeros(3, 8, 8), torch.zeros(pol.config.state_dim)
    got = [float(pol.select_action(img, st, "lift", torch.device("cpu"))[0]) for _ in range(3)]
    assert len(calls) == 3 and len(_FakeEnsembler.made) == 1                       # the backbone on every call, ONE ensembler
    assert got == [100.0, (101.0 + 200.0) / 2, (102.0 + 201.0 + 300.0) / 3]        # uniform weights over the predictions of that time step
    pol.reset()
    assert _FakeEnsembler.made[0]._h is None
    assert float(pol.select_action(img, st, "lift", torch.device("cpu"))[0]) == 400.0 and len(_FakeEnsembler.made) == 2


def test_lerobot_surface_takes_the_option_and_guards_the_batch_size(monkeypatch):
    import fastvla_hip.ensemble as ens_mod
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import HAVE_LEROBOT, FeatureType, PolicyFeature
    if HAVE_LEROBOT:
        pytest.skip("stand-in semantics are only exercised without lerobot")
    monkeypatch.setattr(ens_mod, "TemporalEnsembler", _FakeEnsembler)
    _FakeEnsembler.made.clear()
    feats = {"observation.images.top": PolicyFeature(FeatureType.VISUAL, (3, 96, 96)), "observation.state": PolicyFeature(FeatureType.STATE, (6,))}

    def cfg(**kw):
        return LRConfig(vlm_model_name="synthetic:tiny", hidden_dim=16, fusion_dim=16, input_features=feats,
                        output_features={"action": PolicyFeature(FeatureType.ACTION, (5,))}, **kw)

    with pytest.raises(ValueError, match="n_action_steps"):
        LRPolicy(cfg(chunk_size=4, n_action_steps=2), temporal_ensemble_coeff=0.01)
    assert LRPolicy(cfg(chunk_size=4)).temporal_ensemble_coeff is None
    pol = LRPolicy(cfg(chunk_size=4), temporal_ensemble_coeff=0.0, action_step_weights=[1.0, 1.0, 0.5, 0.0])
    assert pol.temporal_ensemble_coeff == 0.0 and pol.model.action_loss_weights == {"dim": None, "step": [1.0, 1.0, 0.5, 0.0]}
    monkeypatch.setattr(pol.model, "_engine", lambda: "engine")
    calls = []
    pol._predict_actions = lambda b: calls.append(1) or (10.0 * len(calls) + torch.arange(4).float()).view(1, 4, 1).expand(b["n"], 4, 5).clone()
    got = [pol.select_action({"n": 3}) for _ in range(2)]
    assert got[0].shape == (3, 5) and len(calls) == 2 and [float(g[2, 0]) for g in got] == [10.0, (11.0 + 20.0) / 2]
    with pytest.raises(ValueError, match="reset"):
        pol.select_action({"n": 2})                                                # another B without a reset()
    pol.reset()
    assert pol.select_action({"n": 2}).shape == (2, 5) and len(_FakeEnsembler.made) == 2
