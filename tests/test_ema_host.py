"""Host (no GPU): the EMA options, their environment twins, the weight schedule (fastvla_hip/ema.py), the optimiser record and the resume check
(utils/checkpoint.py, fastvla/ema_state.py)."""
import struct
import warnings

import pytest
import torch

from fastvla_hip import ema

F32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]  # noqa: E731
ENV = ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER", "FASTVLA_EMA_SAVE")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def test_schedule_against_hand_written_numbers():
    o = ema.normalize_options()
    assert o == {"decay": 0.999, "warmup": True, "update_after": 0}
    # t = 1 with warm-up: d = (1 + 1) / (10 + 1) = 2/11, w = float32(9/11)
    assert ema.ema_decay(o, 1) == 2.0 / 11.0
    assert ema.ema_weight(o, 1) == F32(1.0 - 2.0 / 11.0) == F32(9.0 / 11.0)
    assert ema.ema_decay(o, 2) == 3.0 / 12.0 and ema.ema_weight(o, 2) == 0.75
    # (1 + tau) / (10 + tau) reaches 0.999 at tau = 8990 (8991 / 9000): the last warm-up value is tau = 8989, 8990 / 8999 < 0.999
    assert ema.ema_decay(o, 8989) == 8990.0 / 8999.0 < 0.999
    assert ema.ema_decay(o, 8990) == 0.999 and ema.ema_decay(o, 10 ** 6) == 0.999
    assert ema.ema_weight(o, 8990) == F32(1.0 - 0.999) == ema.ema_weight(o, 10 ** 6)
    assert ema.ema_weight(o, 8989) == F32(1.0 - 8990.0 / 8999.0) > ema.ema_weight(o, 8990)
    # the float32 weight: the subtraction in double, ONE rounding
    assert ema.ema_weight(o, 8990) == 0.0010000000474974513
    # without warm-up the decay is the decay from the first update
    n = ema.normalize_options(decay=0.99, warmup=False)
    assert ema.ema_weight(n, 1) == ema.ema_weight(n, 500) == F32(1.0 - 0.99)
    # update_after = 3: the average follows the live weights for 3 updates (w = 1), and tau counts from there
    u = ema.normalize_options(decay=0.999, warmup=True, update_after=3)
    assert [ema.ema_weight(u, t) for t in (1, 2, 3)] == [1.0, 1.0, 1.0]
    assert ema.ema_weight(u, 4) == F32(9.0 / 11.0) and ema.ema_weight(u, 5) == 0.75
    ua = ema.normalize_options(decay=0.5, warmup=False, update_after=1)
    assert ema.ema_weight(ua, 1) == 1.0 and ema.ema_weight(ua, 2) == 0.5
    # decay = 0: the average IS the live weights, with and without warm-up
    for wu in (True, False):
        z = ema.normalize_options(decay=0.0, warmup=wu)
        assert ema.ema_weight(z, 1) == 1.0 and ema.ema_weight(z, 77) == 1.0
    with pytest.raises(ValueError):
        ema.ema_weight(o, 0)
    for t in (1, 5, 8989, 8990, 123456):
        w = ema.ema_weight(o, t)
        assert 0.0 < w <= 1.0 and F32(w) == w


def test_value_errors():
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="decay"):
            ema.normalize_options(decay=bad)
    for bad in (-1, 1.5, "x", None, True):
        with pytest.raises(ValueError, match="update_after"):
            ema.normalize_options(update_after=bad)
    for bad in ("yes", 2, None):
        with pytest.raises(ValueError, match="warmup"):
            ema.normalize_options(warmup=bad)
    assert ema.normalize_options(decay="0.9", warmup=0, update_after=2.0) == {"decay": 0.9, "warmup": False, "update_after": 2}


def test_environment_twins_and_explicit_beats_twin(monkeypatch):
    assert ema.options_from_env() is None                        # unset: EMA off
    monkeypatch.setenv("FASTVLA_EMA_WARMUP", "0")
    monkeypatch.setenv("FASTVLA_EMA_UPDATE_AFTER", "5")
    assert ema.options_from_env() is None                        # the decay alone switches it on
    monkeypatch.setenv("FASTVLA_EMA_DECAY", " ")
    assert ema.options_from_env() is None                        # (empty = unset)
    monkeypatch.setenv("FASTVLA_EMA_DECAY", "0.99")
    assert ema.options_from_env() == {"decay": 0.99, "warmup": False, "update_after": 5}
    assert ema.options_from_env({"FASTVLA_EMA_DECAY": "0.5"}) == {"decay": 0.5, "warmup": True, "update_after": 0}
    # an explicit argument beats its twin, option by option
    assert ema.resolve_options() == {"decay": 0.99, "warmup": False, "update_after": 5}
    assert ema.resolve_options(decay=0.9) == {"decay": 0.9, "warmup": False, "update_after": 5}
    assert ema.resolve_options(warmup=True, update_after=0) == {"decay": 0.99, "warmup": True, "update_after": 0}
    assert ema.resolve_options(environ={}) == ema.normalize_options()
    for key, bad in (("FASTVLA_EMA_DECAY", "1.0"), ("FASTVLA_EMA_DECAY", "abc"), ("FASTVLA_EMA_WARMUP", "maybe"), ("FASTVLA_EMA_UPDATE_AFTER", "-2"),
                     ("FASTVLA_EMA_UPDATE_AFTER", "1.5")):
        with pytest.raises(ValueError):
            ema.options_from_env({"FASTVLA_EMA_DECAY": "0.9", key: bad})


def _policy():
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny", hidden_dim=16, fusion_dim=16))


def test_policy_options_and_scope_without_ema(monkeypatch):
    pol = _policy()
    assert not pol.ema_enabled and pol.ema_shadow is None and pol.ema_record() is None
    with pytest.raises(RuntimeError, match="EMA is off"):
        with pol.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="EMA is off"):
        pol.apply_ema()
    monkeypatch.setenv("FASTVLA_EMA_DECAY", "0.9")
    monkeypatch.setenv("FASTVLA_EMA_UPDATE_AFTER", "2")
    assert pol.enable_ema(update_after=0) == {"decay": 0.9, "warmup": True, "update_after": 0}      # explicit beats the twin
    assert pol.ema_enabled and pol.ema_shadow is None          # no trainable buffer on a device yet: the average starts when it exists
    assert pol.enable_ema(update_after=0) == pol._ema["options"]
    with pytest.raises(RuntimeError, match="already running"):
        pol.enable_ema(decay=0.5)
    with pytest.raises(ValueError, match="decay"):
        _policy().enable_ema(decay=1.0)
    pol.disable_ema()
    assert not pol.ema_enabled
    pol._ema_from_env()                                         # after an explicit disable_ema() the twin does not switch it back on
    assert not pol.ema_enabled
    fresh = _policy()
    fresh._ema_from_env()                                       # FASTVLA_EMA_DECAY alone switches it on
    assert fresh.ema_enabled and fresh._ema["options"] == {"decay": 0.9, "warmup": True, "update_after": 2}
    monkeypatch.delenv("FASTVLA_EMA_DECAY")
    off = _policy()
    off._ema_from_env()
    assert not off.ema_enabled


def test_optimizer_record_keys_and_resume_check():
    from vla_fastvlm.utils.checkpoint import check_resume_ema, optimizer_record
    st = {"m": torch.zeros(8), "v": torch.zeros(8), "step": 3}
    plain = optimizer_record(st, None, 5, 3)
    assert sorted(plain) == sorted(["m", "v", "step", "global_step", "update_step"])            # EMA off: exactly the keys it had
    assert sorted(optimizer_record(st, None, 5, 3, ema=None)) == sorted(plain)
    rec = {"options": ema.normalize_options(0.99, True, 1), "shadow": torch.ones(8), "updates": 3}
    with_ema = optimizer_record(st, None, 5, 3, ema=rec)
    assert sorted(with_ema) == sorted(list(plain) + ["ema"]) and sorted(with_ema["ema"]) == ["options", "shadow", "updates"]
    check_resume_ema(rec["options"], ema.normalize_options(0.99, True, 1))
    with pytest.raises(ValueError) as ei:
        check_resume_ema(rec["options"], ema.normalize_options(0.999, True, 1))
    assert "'decay': 0.99," in str(ei.value) and "'decay': 0.999," in str(ei.value)
    with pytest.raises(ValueError, match="update_after"):
        check_resume_ema(rec["options"], ema.normalize_options(0.99, True, 0))
    # a record into a run without EMA: a warning, nothing else
    pol = _policy()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pol.load_ema_record(rec)
    assert len(w) == 1 and "EMA off" in str(w[0].message) and not pol.ema_enabled
    # other options raise, naming both
    pol.enable_ema(decay=0.5, warmup=False, update_after=0)
    with pytest.raises(ValueError) as ei:
        pol.load_ema_record(rec)
    assert "'decay': 0.99," in str(ei.value) and "'decay': 0.5," in str(ei.value)
