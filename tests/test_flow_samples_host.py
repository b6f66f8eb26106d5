"""CPU: several samples per observation, one chosen -- the reference's own properties, the weight schedule, the host-side refusals, the two-mode toy, and
the fp32 emulation's distance from float64 on every case the GPU test runs (tests/test_gpu_flow_samples.py calibrates its bar on it).

The toy's bars come from the binomial, not from the figures: with 8 candidates a row lacks a + candidate with probability 2^-8, so the coherent fraction is
1 - 2^-8 = 0.996 in expectation with sigma = sqrt(2^-8 / 512) = 0.003 over 512 rows (bar 0.97); one sample lands in + half the time, sigma = 0.022 (bar
0.4 .. 0.6); the medoid of a row lies IN a mode, |x| = 1 (bar 0.9); the mean of eight has E|2 Bin(8, 1/2) / 8 - 1| = 0.273 (bar 0.5)."""
import numpy as np
import pytest

import flow_samples_util as sm
from fastvla_hip import select as sel


# ------------------------------------------------------------------------------------------------------------------ the reference's own properties
def test_duplicates_tie_and_the_lower_index_wins():
    g = np.random.default_rng(1)
    cand = g.standard_normal((5, 7, 12))
    prev = g.standard_normal((7, 12))
    cand[3] = cand[1]
    for select, kw in (("medoid", {}), ("coherent", dict(prev=prev, shift=1, K=4, w=sm.weights(4)))):
        sc, ch, _ = sm.select_ref(cand, select, **kw)
        assert np.array_equal(sc[:, 1], sc[:, 3]) and bool((ch != 3).all())
    # a winner and its copy: the copy behind it loses, the copy in front of it wins
    _, ch, _ = sm.select_ref(cand, "coherent", prev=prev, shift=0, K=4, w=sm.weights(4))
    swapped = cand.copy()
    rows = np.arange(7)
    swapped[4] = cand[ch, rows]
    assert np.array_equal(sm.select_ref(swapped, "coherent", prev=prev, shift=0, K=4, w=sm.weights(4))[1][ch < 4], ch[ch < 4])
    swapped = cand.copy()
    swapped[0] = cand[ch, rows]
    assert bool((sm.select_ref(swapped, "coherent", prev=prev, shift=0, K=4, w=sm.weights(4))[1] == 0).all())


def test_permuting_the_candidates_moves_the_choice_with_them():
    g = np.random.default_rng(2)
    cand, prev = g.standard_normal((6, 9, 20)), g.standard_normal((9, 20))
    perm = g.permutation(6)
    for select, kw in (("medoid", {}), ("coherent", dict(prev=prev, shift=2, K=5, w=sm.weights(5)))):
        sc, ch, sp = sm.select_ref(cand, select, **kw)
        sc2, ch2, sp2 = sm.select_ref(cand[perm], select, **kw)
        assert np.array_equal(perm[ch2], ch) and np.allclose(sc2, sc[:, perm], rtol=1e-12) and np.allclose(sp, sp2, rtol=1e-12)
    assert bool((sm.select_ref(cand, "first")[1] == 0).all())


def test_special_scores():
    g = np.random.default_rng(3)
    cand, prev = g.standard_normal((4, 5, 12)), g.standard_normal((5, 12))
    kw = dict(prev=prev, K=4, w=sm.weights(4))
    assert bool((sm.select_ref(cand, "coherent", shift=4, **kw)[1] == 0).all())                          # no overlap: candidate 0
    assert bool((sm.select_ref(cand, "coherent", shift=0, prev=prev, K=4, w=np.zeros(4))[1] == 0).all())      # all-zero weights: candidate 0
    mask = np.array([1, 0, 1, 0, 0])
    sc, ch, _ = sm.select_ref(cand, "coherent", shift=1, row_mask=mask, **kw)
    msc, mch, _ = sm.select_ref(cand, "medoid")
    assert np.array_equal(ch[mask == 0], mch[mask == 0]) and np.array_equal(sc[mask == 0], msc[mask == 0])
    bad = cand.copy()
    bad[2, :, 5] = np.nan
    for select, k in (("medoid", {}), ("coherent", dict(shift=1, **kw))):
        sc, ch, _ = sm.select_ref(bad, select, **k)
        assert bool(np.isinf(sc[:, 2]).all() and np.isfinite(np.delete(sc, 2, axis=1)).all() and (ch != 2).all())
    bad[:, :, 0] = np.inf
    assert bool((sm.select_ref(bad, "medoid")[1] == 0).all())
    nanprev = prev.copy()
    nanprev[:, :3] = np.nan                                                                              # beyond the overlap at shift 1
    assert np.array_equal(sm.select_ref(cand, "coherent", shift=1, prev=nanprev, K=4, w=sm.weights(4))[0], sm.select_ref(cand, "coherent", shift=1, **kw)[0])


# ------------------------------------------------------------------------------------------------------------------ the schedule and the refusals
def test_coherence_weights():
    assert sel.coherence_weights(4, 0.5) == [1.0, 0.5, 0.25, 0.125] and sel.coherence_weights(3, 1.0) == [1.0, 1.0, 1.0]
    assert sel.coherence_weights(50)[49] == 0.5 ** 49
    for K, decay in ((0, 0.5), (True, 0.5), (2.0, 0.5), (4, 0.0), (4, 1.5), (4, -0.5), (4, float("nan"))):
        with pytest.raises(ValueError):
            sel.coherence_weights(K, decay)


def test_check_flow_samples_and_select():
    assert [sel.check_flow_samples(s) for s in (1, 2, 16)] == [1, 2, 16]
    for s in (0, 17, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="flow_samples"):
            sel.check_flow_samples(s)
    assert sel.check_flow_select(None, None) == (1, None) and sel.check_flow_select(1, None) == (1, None)
    assert sel.check_flow_select(4, None) == (4, "medoid") and sel.check_flow_select(4, "coherent", chunk_size=8, rtc_method="prefix") == (4, "coherent")
    assert sel.check_flow_select(None, None, action_head="regression") == (1, None)
    both = "flow_samples.*flow_select|flow_select.*flow_samples"
    for args, kw, match in (((4, None), dict(action_head="regression"), "flow_samples.*action_head"), ((None, "medoid"), dict(action_head="regression"), "flow_select.*action_head"),
                            ((17, "medoid"), {}, "flow_samples"), ((0, None), {}, "flow_samples"), ((1, "medoid"), {}, both), ((None, "first"), {}, both),
                            ((4, "mean"), {}, both), ((4, "coherent"), dict(chunk_size=1), both + "|flow_select.*chunk_size"),
                            ((4, "medoid"), dict(rtc_method="guidance"), "flow_samples.*rtc_method")):
        with pytest.raises(ValueError, match=match):
            sel.check_flow_select(*args, **kw)


# ------------------------------------------------------------------------------------------------------------------ the toy
def test_two_mode_toy_chosen_candidates_stay_in_a_mode_and_the_mean_does_not():
    f = sm.toy_figures()
    print(f"[flow samples toy] {f}")
    assert f["coherent_plus"] >= 0.97 and 0.4 <= f["single_plus"] <= 0.6
    assert f["coherent_plus"] == pytest.approx(1.0 - f["rows_without_plus"] / 512)      # it misses exactly the rows that have no + candidate
    assert f["medoid_mean_abs"] >= 0.9 and f["mean_mean_abs"] <= 0.5


# ------------------------------------------------------------------------------------------------------------------ the emulation's distance
def test_emulation_stays_within_the_fp32_sum_bar_on_every_gpu_case():
    worst = 0.0
    for name in sm.HEADS:
        for select in ("medoid", "coherent"):
            d_sc, d_sp = sm.emulation_distance(name, select)
            print(f"[flow samples emulation {name} {select}] scores {d_sc:.3e}, spread {d_sp:.3e}")
            assert 0.0 < d_sc < 1e-5 and 0.0 < d_sp < 1e-5
            worst = max(worst, d_sc, d_sp)
    assert worst < 1e-5


def test_near_ties_of_the_random_cases_stay_within_the_cap():
    left_out = rows = 0
    for name, B, S in sm.RANDOM_CASES:
        c = sm.random_case(name, B, S)
        for select in ("medoid", "coherent"):
            if select == "medoid" and S == 2:
                continue                    # an exact tie by construction: the GPU test asserts candidate 0 there
            sc, _, _ = sm.select_ref(c["cand"], select, **sm.case_kwargs(c, select))
            decided = sm.decided_rows(sc, 4 * sm.emulation_distance(name, select)[0])
            left_out, rows = left_out + int((~decided).sum()), rows + B
    print(f"[flow samples near ties] {left_out} of {rows} rows lie within the bar")
    assert left_out <= sm.NEAR_TIE_CAP * rows


def test_exact_cases_are_exact_in_fp32():
    for name in sm.HEADS:
        for B, S in ((1, 2), (9, 16)):
            c = sm.exact_case(name, B, S)
            for select in ("medoid", "coherent"):
                for shift in (sm.SHIFTS(c["K"]) if select == "coherent" else (0,)):
                    kw = sm.case_kwargs(c, select, shift=shift)
                    sc64 = sm.select_ref(c["cand"], select, **kw)[0]
                    sc32 = sm.select_emu32(c["cand"], select, **kw)[0]
                    assert np.array_equal(sc32.astype(np.float64), sc64) and float(sc64.max()) < 2 ** 24


# ------------------------------------------------------------------------------------------------------------------ both policy surfaces, no GPU
SAMPLES_ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_SAMPLES", "FASTVLA_FLOW_SELECT", "FASTVLA_FLOW_COHERENCE_DECAY", "FASTVLA_RTC", "FASTVLA_RTC_METHOD",
               "FASTVLA_FLOW_PREFIX_MAX_DELAY", "FASTVLA_FLOW_SOLVER", "FASTVLA_FLOW_NOISE_DRAWS", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "FASTVLA_CHUNK_SIZE")
FLOW = dict(action_head="flow", flow_time_dim=6, flow_steps=4, flow_seed=9)


def _core(chunk_size=3, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=chunk_size, **kw)


def _plugin(**kw):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=4, n_action_steps=2,
                   output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(5,))}, dropout=0.0)
    return LRPolicy(cfg, **kw)


@pytest.mark.parametrize("make", [_core, _plugin])
def test_policy_arguments_twins_and_refusals(monkeypatch, make):
    """no engine is built: every setting is resolved and refused in the constructor"""
    import dataclasses
    for k in SAMPLES_ENV:
        monkeypatch.delenv(k, raising=False)
    off = make(**FLOW)
    assert (off.flow_samples, off.flow_select) == (1, None) and off.model.backbone.head_spec.samples is None and off.last_candidates is None
    med = make(**FLOW, flow_samples=4)
    assert (med.flow_samples, med.flow_select) == (4, "medoid") and med.model.backbone.head_spec.samples == dict(max_samples=4, step_weights=None)
    coh = make(**FLOW, flow_samples=5, flow_select="coherent", flow_coherence_decay=0.25)
    K = coh.model.chunk_size
    assert coh.model.backbone.head_spec.samples == dict(max_samples=5, step_weights=[0.25 ** k for k in range(K)])
    assert make(**FLOW, flow_samples=2, flow_select="first").flow_select == "first"
    # a property of the run: no record anywhere
    assert med.model.flow_record() == off.model.flow_record() and coh.model.flow_record() == off.model.flow_record()
    assert not any("sample" in f.name or "select" in f.name for f in dataclasses.fields(type(_plugin().config)))      # the registered config gains no field
    # with rtc_method="prefix" it works; with guidance it is refused
    pre = make(**FLOW, flow_samples=3, flow_select="coherent", rtc=True, rtc_method="prefix", flow_prefix_max_delay=1)
    assert pre.flow_samples == 3 and pre.rtc["method"] == "prefix"
    for kw, match in ((dict(flow_samples=4), "flow_samples.*action_head"), (dict(flow_select="medoid"), "flow_select.*action_head"),
                      (dict(**FLOW, flow_samples=17), "flow_samples"), (dict(**FLOW, flow_samples=0), "flow_samples"),
                      (dict(**FLOW, flow_select="medoid"), "flow_select.*flow_samples"), (dict(**FLOW, flow_samples=1, flow_select="first"), "flow_select.*flow_samples"),
                      (dict(**FLOW, flow_samples=4, flow_select="mean"), "flow_select.*flow_samples"),
                      (dict(**FLOW, flow_samples=4, rtc=True), "flow_samples.*rtc_method"), (dict(**FLOW, flow_samples=4, flow_coherence_decay=0.0), "flow_coherence_decay"),
                      (dict(flow_coherence_decay=0.5), "flow_coherence_decay.*action_head")):
        with pytest.raises(ValueError, match=match):
            make(**kw)
    # the twins, read for a flow head only; an argument beats them
    monkeypatch.setenv("FASTVLA_FLOW_SAMPLES", "6")
    monkeypatch.setenv("FASTVLA_FLOW_SELECT", "Coherent")
    monkeypatch.setenv("FASTVLA_FLOW_COHERENCE_DECAY", "0.75")
    tw = make(**FLOW)
    assert (tw.flow_samples, tw.flow_select) == (6, "coherent") and tw.model.backbone.head_spec.samples["step_weights"][1] == 0.75
    assert make(**FLOW, flow_samples=2, flow_select="first").flow_samples == 2
    reg = make()
    assert (reg.flow_samples, reg.flow_select) == (1, None)
    monkeypatch.setenv("FASTVLA_FLOW_SAMPLES", "many")
    assert make().flow_samples == 1
    with pytest.raises(ValueError, match="FASTVLA_FLOW_SAMPLES"):
        make(**FLOW)


def test_coherent_needs_more_than_one_step(monkeypatch):
    for k in SAMPLES_ENV:
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(ValueError, match="flow_select.*chunk_size|chunk_size.*flow_select"):
        _core(chunk_size=1, **FLOW, flow_samples=4, flow_select="coherent")
    assert _core(chunk_size=1, **FLOW, flow_samples=4).flow_select == "medoid"


def test_num_samples_is_bounded_by_the_constructed_count(monkeypatch):
    import torch
    for k in SAMPLES_ENV:
        monkeypatch.delenv(k, raising=False)
    pol = _core(**FLOW, flow_samples=4)
    for bad in (5, 0, True, 2.0):
        with pytest.raises(ValueError, match="num_samples|flow_samples"):
            pol.select_action_chunk(torch.zeros(3, 64, 64), torch.zeros(14), "t", torch.device("cpu"), num_samples=bad)
    assert pol.model.flow_samples_now == 4
