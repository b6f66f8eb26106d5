"""CPU: the binned action head's options -- constructor keyword or FASTVLA_ACTION_BINS* twin -> resolve_policy_options -> PolicyOptions -> HeadSpec -> the
set_head_bins call of HeadSpec.apply -- on both policy surfaces, every refusal before any engine exists, the hip_extras.json record, and the properties of the
float64 HL-Gauss reference the GPU tests compare against.  No engine is built."""
import json
import os

import numpy as np
import pytest
import torch

from action_bins_util import bins_ref, bins_table, per_element, target_dist, target_index


@pytest.fixture(autouse=True)
def _no_twins(monkeypatch):
    for k in [k for k in os.environ if k.startswith("FASTVLA_")]:
        monkeypatch.delenv(k)


A = 5


def _core(K=3, n=2, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", state_dim=6, action_dim=A, hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K,
                         n_action_steps=n, **kw)


def _plugin(K=3, n=2, **kw):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, input_features=feats, chunk_size=K, n_action_steps=n,
                   output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
    return LRPolicy(cfg, **kw)


SURFACES = (_core, _plugin)
PER_DIM = [(-1.0, 1.0), (-2.0, 2.0), (-3.0, 3.0), (-0.5, 0.5), (0.0, 1.0)]


@pytest.mark.parametrize("make", SURFACES)
def test_keywords_resolve_into_the_head_spec(make):
    pol = make(action_head="bins", action_bins=64, action_bins_range=PER_DIM, action_bins_sigma=0.75, action_bins_decode="mean")
    want = dict(bins=64, range=[[float(lo), float(hi)] for lo, hi in PER_DIM], sigma=0.75, decode="mean")
    assert pol.action_head == "bins" and pol.options.bins == want and pol.model.bins == want and pol.model.backbone.head_spec.bins == want
    assert pol.model.backbone._engine is None                                  # resolved without an engine
    assert tuple(pol.model.action_head.weight.shape) == (3 * A * 64, 64) and tuple(pol.model.action_head.bias.shape) == (3 * A * 64,)
    assert pol.model.backbone.head_spec.dims["action_dim"] == 3 * A           # the ACTION width stays K * A
    assert pol.model.flow is None and pol.model.flow_record() == {"type": "bins", **want}
    # the defaults: 256 bins over (-3, 3), one-hot targets, argmax
    d = make(action_head="bins")
    assert d.options.bins == dict(bins=256, range=[[-3.0, 3.0]], sigma=0.0, decode="argmax")
    # HeadSpec.apply: ONE call, ahead of the loss setters
    calls = []

    class Stub:
        def __getattr__(self, name):
            return lambda *a, **k: calls.append((name, a, k))

    pol.model.backbone.head_spec.apply(Stub())
    assert calls[0] == ("set_head_bins", (), want) and [c[0] for c in calls] == ["set_head_bins", "set_head_loss"]


@pytest.mark.parametrize("make", SURFACES)
def test_twins_are_read_for_a_bins_head_only(monkeypatch, make):
    for k, v in (("FASTVLA_ACTION_BINS", "32"), ("FASTVLA_ACTION_BINS_RANGE", "-2:1.5"), ("FASTVLA_ACTION_BINS_SIGMA", "0.5"), ("FASTVLA_ACTION_BINS_DECODE", "MEAN")):
        monkeypatch.setenv(k, v)
    plain, flow = make(), make(action_head="flow", flow_steps=2, flow_time_dim=6)
    assert plain.options.bins is None and plain.action_head == "regression" and flow.options.bins is None and flow.model.bins is None
    assert tuple(plain.model.action_head.weight.shape) == (3 * A, 64)
    monkeypatch.setenv("FASTVLA_ACTION_HEAD", "bins")
    pol = make()
    assert pol.options.bins == dict(bins=32, range=[[-2.0, 1.5]], sigma=0.5, decode="mean")
    assert make(action_bins=16, action_bins_decode="argmax").options.bins == dict(bins=16, range=[[-2.0, 1.5]], sigma=0.5, decode="argmax")   # an argument beats its twin
    # stray garbage in a twin cannot make a policy with another head raise
    monkeypatch.setenv("FASTVLA_ACTION_HEAD", "regression")
    monkeypatch.setenv("FASTVLA_ACTION_BINS", "many")
    monkeypatch.setenv("FASTVLA_ACTION_BINS_RANGE", "wide")
    assert make().options.bins is None
    monkeypatch.setenv("FASTVLA_ACTION_HEAD", "bins")
    with pytest.raises(ValueError, match="FASTVLA_ACTION_BINS"):
        make()


REFUSALS = [
    (dict(action_head="bins", flow_steps=4), ("flow_steps", "action_head='bins'")),
    (dict(action_head="bins", flow_time_dim=8), ("flow_time_dim", "action_head='bins'")),
    (dict(action_head="bins", flow_time_dist="logit_normal"), ("flow_time_dist", "action_head='bins'")),
    (dict(action_head="bins", flow_time_range=(0.1, 0.9)), ("flow_time_range", "action_head='bins'")),
    (dict(action_head="bins", flow_time_stratify=True), ("flow_time_stratify", "action_head='bins'")),
    (dict(action_head="bins", flow_seed=3), ("flow_seed", "action_head='bins'")),
    (dict(action_head="bins", flow_noise_draws=2), ("flow_noise_draws", "action_head='bins'")),
    (dict(action_head="bins", flow_solver="heun"), ("flow_solver", "action_head='bins'")),
    (dict(action_head="bins", flow_prefix_max_delay=1), ("flow_prefix_max_delay", "action_head='bins'")),
    (dict(action_head="bins", flow_samples=2), ("flow_samples", "action_head='bins'")),
    (dict(action_head="bins", flow_select="medoid"), ("flow_select", "action_head='bins'")),
    (dict(action_head="bins", rtc=True), ("rtc", "action_head='bins'")),
    (dict(action_head="bins", rtc_schedule="exp"), ("rtc_schedule", "action_head='bins'")),
    (dict(action_head="bins", rtc_method="prefix"), ("rtc_method", "action_head='bins'")),
    (dict(action_bins=64), ("action_bins=64", "action_head='regression'")),
    (dict(action_bins_range=(-1, 1)), ("action_bins_range", "action_head='regression'")),
    (dict(action_bins_sigma=0.75), ("action_bins_sigma", "action_head='regression'")),
    (dict(action_bins_decode="mean"), ("action_bins_decode", "action_head='regression'")),
    (dict(action_head="flow", flow_time_dim=6, action_bins=64), ("action_bins=64", "action_head='flow'")),
    (dict(action_head="bins", action_bins=1), ("action_bins=1", "2 .. 1024")),
    (dict(action_head="bins", action_bins=1025), ("action_bins=1025", "2 .. 1024")),
    (dict(action_head="bins", action_bins=2.5), ("action_bins=2.5", "2 .. 1024")),
    (dict(K=8, action_head="bins", action_bins=1024), ("chunk_size=8", "action_dim=5", "action_bins=1024", "32768")),      # 8 * 5 * 1024 = 40960
    (dict(action_head="bins", action_bins_range=(1.0, 1.0)), ("lo=1.0", "hi=1.0")),
    (dict(action_head="bins", action_bins_range=(2.0, -2.0)), ("lo=2.0", "hi=-2.0")),
    (dict(action_head="bins", action_bins_range=(0.0, float("inf"))), ("lo=0.0", "hi=inf")),
    (dict(action_head="bins", action_bins_range=[(-1, 1)] * 3), ("3 pairs", "action_dim=5")),
    (dict(action_head="bins", action_bins_range=[(-1, 1)] * 15), ("15 pairs", "action_dim=5")),
    (dict(action_head="bins", action_bins_sigma=-0.5), ("action_bins_sigma=-0.5", "action_bins=256")),
    (dict(action_head="bins", action_bins_sigma=float("nan")), ("action_bins_sigma=nan", "action_bins=256")),
    (dict(action_head="bins", action_bins_decode="median"), ("action_bins_decode='median'", "action_head='bins'")),
]


@pytest.mark.parametrize("make", SURFACES)
@pytest.mark.parametrize("kw,parts", REFUSALS, ids=[", ".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_refusals_name_both_settings_before_any_engine_exists(monkeypatch, make, kw, parts):
    import fastvla_hip.engine as E
    monkeypatch.setattr(E.FastVLAEngine, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was built")))
    with pytest.raises(ValueError) as ei:
        make(**kw)
    assert make(8, 2, action_head="bins", action_bins=819).options.bins["bins"] == 819      # 8 * 5 * 819 = 32760: the widest head that fits
    for part in parts:
        assert part in str(ei.value), (part, str(ei.value))


def test_bins_refuse_another_loss_kind(monkeypatch):
    with pytest.raises(ValueError) as ei:
        _core(action_head="bins", action_loss="l1")
    assert "action_loss='l1'" in str(ei.value) and "action_head='bins'" in str(ei.value)
    monkeypatch.setenv("FASTVLA_ACTION_LOSS", "smooth_l1")                    # the LeRobot surface takes the kind from the twin
    with pytest.raises(ValueError) as ei:
        _plugin(action_head="bins")
    assert "action_loss='smooth_l1'" in str(ei.value) and "action_head='bins'" in str(ei.value)
    monkeypatch.delenv("FASTVLA_ACTION_LOSS")
    pol = _core(action_head="bins", action_bins=8)
    with pytest.raises(ValueError, match="action_loss"):                      # ... and later, through set_action_loss
        pol.set_action_loss("l1")
    assert pol.model.action_loss == "mse"


def test_predict_under_autograd_is_refused():
    pol = _core(action_head="bins", action_bins=8)
    pol.model.materialize = lambda device=None: None                          # (no engine: the refusal comes before the head runs)
    with pytest.raises(ValueError) as ei:
        pol.model.head(torch.zeros(2, 8), torch.zeros(2, 6))
    assert "action_head='bins'" in str(ei.value) and "autograd" in str(ei.value)


def test_checkpoint_record_and_cross_type_load_error(tmp_path):
    from vla_fastvlm.utils.checkpoint import check_action_head_shape, check_head_width, flow_kwargs, save_policy_checkpoint
    torch.manual_seed(0)
    pol = _core(action_head="bins", action_bins=16, action_bins_range=PER_DIM, action_bins_sigma=0.75, action_bins_decode="mean")
    d = save_policy_checkpoint(pol, tmp_path / "ck")
    ex = json.loads((d / "hip_extras.json").read_text())
    rec = {"type": "bins", "bins": 16, "range": [[float(lo), float(hi)] for lo, hi in PER_DIM], "sigma": 0.75, "decode": "mean"}
    assert ex["action_head"] == rec and ex["action_chunk"]["chunk_size"] == 3
    kw = flow_kwargs(rec)
    assert kw == dict(action_head="bins", action_bins=16, action_bins_range=[tuple(map(float, p)) for p in PER_DIM], action_bins_sigma=0.75, action_bins_decode="mean")
    again = _core(**kw)
    assert again.options.bins == pol.options.bins
    state = torch.load(d / "policy_state_dict.pt")
    assert tuple(state["model.action_head.weight"].shape) == (3 * A * 16, 64)
    check_head_width(state, A, ex["action_chunk"], d, ex["action_head"])
    check_action_head_shape(state, again, d)
    with pytest.raises(ValueError, match="action_head.weight"):              # the record is missing: a tall head does not load as a regression head
        check_head_width(state, A, ex["action_chunk"], d, None)
    for other in (_core(), _core(action_head="flow", flow_time_dim=6), _core(action_head="bins", action_bins=8)):
        with pytest.raises(ValueError) as ei:
            check_action_head_shape(state, other, d)
        assert "model.action_head.weight" in str(ei.value) and "(240, 64)" in str(ei.value) and str(tuple(other.model.action_head.weight.shape)) in str(ei.value)
    plain = {"model.action_head.weight": torch.zeros(3 * A, 64)}
    with pytest.raises(ValueError) as ei:
        check_action_head_shape(plain, pol, "x")
    assert "(15, 64)" in str(ei.value) and "(240, 64)" in str(ei.value)
    # a default policy's files gain nothing
    d0 = save_policy_checkpoint(_core(1, 1), tmp_path / "plain")
    assert not (d0 / "hip_extras.json").is_file() or "action_head" not in json.loads((d0 / "hip_extras.json").read_text())


def test_ranges_from_dataset_statistics():
    from fastvla_hip.engine import bins_ranges_from_stats, check_head_bins
    stats = {"min": [-1.0, 0.0, 5.0], "max": [3.0, 10.0, 5.0], "mean": [1.0, 5.0, 5.0], "std": [2.0, 2.5, 0.0]}
    r = bins_ranges_from_stats(stats, margin=0.0)
    assert r[0] == (-1.0, 1.0) and r[1] == (-2.0, 2.0) and r[2] == (-1.0, 1.0)          # (a - mean) / std of the extremes; a constant dimension gets (-1, 1)
    r = bins_ranges_from_stats(stats, margin=0.25)
    assert r[0] == (-1.5, 1.5) and r[1] == (-3.0, 3.0)
    assert bins_ranges_from_stats(stats, mode="std", num_std=2.5) == [(-2.5, 2.5)] * 3
    assert check_head_bins(32, r, 0.0, "argmax", 3, 2)["range"] == [[-1.5, 1.5], [-3.0, 3.0], [-1.0, 1.0]]
    with pytest.raises(ValueError):
        bins_ranges_from_stats(stats, mode="quantile")


# ---------------------------------------------------------------------------------------------------------------- the float64 reference itself
@pytest.mark.parametrize("nb,rng", [(2, (-1.0, 1.0)), (64, (-3.0, 3.0)), (96, (-3.0, 3.0)), (256, (-0.7, 2.3)), (1000, (-3.0, 3.0))])
def test_hl_gauss_reference_properties(nb, rng):
    table = bins_table(rng, nb, 1)
    lo, hi, w = (float(v[0]) for v in table)
    g = torch.Generator().manual_seed(nb)
    t = (lo - 0.2 * (hi - lo) + 1.4 * (hi - lo) * torch.rand(257, generator=g, dtype=torch.float64)).numpy()
    t[:3] = (lo, hi, 0.5 * (lo + hi))
    a, idx = target_index(t, lo, hi, w, nb)
    centres = lo + (np.arange(nb) + 0.5) * w
    for sigma in (0.25, 0.75, 2.0):
        q = target_dist(t, lo, hi, w, nb, sigma)
        assert q.shape == (257, nb) and bool((q >= 0).all())
        assert float(np.abs(q.sum(-1) - 1.0).max()) <= 1e-12                  # sum q = 1 (the edge CDFs telescope; the last edge is hi)
        # the mean of q lies within one bin width of the clamped target: w / 2 from reading each bin at its centre, and at the ends of the range, where the
        # Gaussian is cut in half, sigma w sqrt(2 / pi) more -- below w up to the recommended sigma = 0.75 (a wider one pulls a target at the boundary further in)
        if sigma <= 0.75:
            assert float(np.abs((q * centres).sum(-1) - a).max()) <= w
    one_hot = target_dist(t, lo, hi, w, nb, 0.0)
    assert bool((one_hot.sum(-1) == 1).all()) and bool((np.argmax(one_hot, -1) == idx).all())
    # sigma -> 0 tends to the one-hot (targets at bin centres: the mass outside the bin is 2 Phi(-1 / (2 sigma)))
    tc = centres[:: max(1, nb // 17)]
    for sigma, bar in ((0.25, 2 * 0.0228), (0.125, 1e-4), (0.05, 1e-12)):
        q = target_dist(tc, lo, hi, w, nb, sigma)
        _, ic = target_index(tc, lo, hi, w, nb)
        assert float((1.0 - np.take_along_axis(q, ic[:, None], -1)).max()) <= bar, sigma
    # the loss of the reference at its own optimum p = q is the entropy of q, and the gradient vanishes there
    q = target_dist(t[:8], lo, hi, w, nb, 0.75)
    z = np.log(np.maximum(q, 1e-300)).reshape(8, 1, 1, nb)
    r = bins_ref(z, t[:8].reshape(8, 1, 1), table, sigma=0.75)
    ent = float(-(np.where(q > 0, q * np.log(np.maximum(q, 1e-300)), 0.0)).sum() / 8)
    assert abs(r["loss"] - ent) <= 1e-12 * max(1.0, ent) and float(np.abs(r["g"]).max()) <= 1e-15


def test_reference_selects_masked_targets_away():
    table = bins_table([(-1, 1), (-2, 2)], 8, 4)
    lo, hi, w = per_element(table, 2, 2)
    assert lo.tolist() == [[-1, -2], [-1, -2]] and w.tolist() == [[0.25, 0.5], [0.25, 0.5]]          # element e = k A + a reads pair e % 2
    g = torch.Generator().manual_seed(1)
    z = torch.randn(3, 2, 2, 8, generator=g, dtype=torch.float64).numpy()
    t = torch.randn(3, 2, 2, generator=g, dtype=torch.float64).numpy()
    pad = np.array([[0, 1], [0, 0], [1, 1]], dtype=bool)
    poisoned = t.copy()
    poisoned[pad] = np.nan
    poisoned[:, :, 1] = np.inf                                                # dimension 1 has weight 0
    a = bins_ref(z, poisoned, table, pad=pad, sigma=0.75, dim_w=[1.0, 0.0], step_w=[1.0, 2.0])
    t2 = np.where(a["live"], t, 0.0)
    b = bins_ref(z, t2, table, pad=pad, sigma=0.75, dim_w=[1.0, 0.0], step_w=[1.0, 2.0])
    assert np.isfinite(a["loss"]) and a["loss"] == b["loss"] and np.array_equal(a["g"], b["g"]) and bool((a["g"][~a["live"]] == 0).all())
    assert a["valid"] == 0.5 and a["nvalid"] == 6
