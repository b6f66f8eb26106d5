"""CPU: the step guard's host half -- the reference state machine of tests/step_guard_util.py on scripted sequences, the options of fastvla_hip/guard.py with
their environment twins and refusals, the optimizer.pt key, and the flag's all-reduce on two gloo ranks."""
import math
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fastvla_hip import guard
from step_guard_util import GuardRef

ENV_KEYS = ["FASTVLA_STEP_GUARD"] + [f"FASTVLA_STEP_GUARD_{k.upper()}" for k in guard.OPTION_KEYS]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ the reference state machine
def test_growth_at_exactly_growth_interval():
    r = GuardRef(init_delta_log2=-2, min_delta_log2=-4, max_delta_log2=4, growth_interval=3)
    for i in (1, 2):
        assert r.step(1.0) and (r.delta_log2, r.good_steps) == (-2, i)
    assert r.step(1.0) and (r.delta_log2, r.good_steps) == (-1, 0)           # the third good step grows, and the run starts over
    assert r.step(1.0) and (r.delta_log2, r.good_steps) == (-1, 1)
    assert r.as_export()["last_inv_delta"] == 2.0 and r.applied == 4        # the step ran with the delta it was computed under, 2^-1


def test_a_skip_resets_the_run_of_good_steps():
    r = GuardRef(init_delta_log2=0, min_delta_log2=-4, max_delta_log2=4, growth_interval=3)
    assert r.step(1.0) and r.step(1.0) and r.good_steps == 2
    assert not r.step(math.inf) and (r.delta_log2, r.good_steps, r.skipped_nonfinite) == (-1, 0, 1)
    assert r.step(1.0) and r.step(1.0) and r.delta_log2 == -1
    assert r.step(1.0) and r.delta_log2 == 0


def test_backoff_is_clamped_at_the_floor_and_growth_at_the_ceiling():
    r = GuardRef(init_delta_log2=-1, min_delta_log2=-2, max_delta_log2=1, growth_interval=1, backoff_log2=3, growth_log2=2)
    assert not r.step(math.nan) and r.delta_log2 == -2                       # -1 - 3 clamps at the floor
    assert not r.step(-math.inf) and r.delta_log2 == -2 and r.skipped_nonfinite == 2       # a non-finite norm skips at the floor too
    assert r.step(4.0) and r.delta_log2 == 0
    assert r.step(4.0) and r.delta_log2 == 1                                 # 0 + 2 clamps at the ceiling
    assert r.step(4.0) and r.delta_log2 == 1 and r.applied == 3


def test_a_flag_above_the_floor_skips_and_at_the_floor_is_applied():
    r = GuardRef(init_delta_log2=1, min_delta_log2=0, max_delta_log2=4, growth_interval=100)
    r.observe(7)
    assert r.flag == 1 and r.last_saturations == 7
    r.observe(7)                                                             # the same count again: no news, and the flag stays (sticky)
    assert r.flag == 1
    assert not r.step(1.0) and (r.delta_log2, r.skipped_saturated, r.flag) == (0, 1, 0)
    r.observe(9)
    assert r.step(1.0) and (r.delta_log2, r.saturated_applied, r.applied, r.skipped_saturated, r.flag) == (0, 1, 1, 1, 0)
    r.set_flag(2)                                                            # (what a sum over two ranks leaves)
    assert not r.step(math.inf) and r.skipped_nonfinite == 1 and r.skipped_saturated == 1 and r.flag == 0      # non-finite wins the count


def test_skip_on_saturation_off_applies_a_flagged_step():
    r = GuardRef(init_delta_log2=2, min_delta_log2=0, max_delta_log2=4, growth_interval=100, skip_on_saturation=False)
    r.set_flag()
    assert r.step(1.0) and (r.delta_log2, r.saturated_applied, r.skipped_saturated) == (2, 1, 0)


# ------------------------------------------------------------------------------------------------ options
def test_defaults_and_value_errors():
    assert guard.normalize_options() == guard.DEFAULTS == {"dynamic_loss_scale": True, "growth_interval": 2000, "backoff_log2": 1, "growth_log2": 1,
                                                           "min_loss_scale_log2": 0, "max_loss_scale_log2": 24}
    for kw in (dict(growth_interval=0), dict(growth_interval=2.5), dict(growth_interval="many"), dict(backoff_log2=-1), dict(growth_log2=-1),
               dict(min_loss_scale_log2=-1), dict(max_loss_scale_log2=25), dict(dynamic_loss_scale="yes"), dict(growth_interval=True)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            guard.normalize_options(**kw)
    with pytest.raises(ValueError) as ei:
        guard.normalize_options(min_loss_scale_log2=14, max_loss_scale_log2=10)
    assert "min_loss_scale_log2=14" in str(ei.value) and "max_loss_scale_log2=10" in str(ei.value)


def test_guard_config_from_options_and_loss_scale():
    o = guard.normalize_options(min_loss_scale_log2=4, max_loss_scale_log2=16, growth_interval=7)
    c = guard.guard_config(o, 12)
    assert (c["init_delta_log2"], c["min_delta_log2"], c["max_delta_log2"], c["growth_interval"], c["skip_on_saturation"]) == (0, -8, 4, 7, True)
    pinned = guard.guard_config(guard.normalize_options(dynamic_loss_scale=False), 12)
    assert (pinned["init_delta_log2"], pinned["min_delta_log2"], pinned["max_delta_log2"]) == (0, 0, 0)
    head = guard.guard_config(o, None)                                      # head-only: fp32, no loss scale, delta stays 1
    assert (head["min_delta_log2"], head["max_delta_log2"]) == (0, 0)
    with pytest.raises(ValueError) as ei:
        guard.guard_config(o, 2)
    assert "loss_scale_log2=2" in str(ei.value) and "min_loss_scale_log2=4" in str(ei.value)


def test_environment_twins_and_explicit_beats_twin(monkeypatch):
    assert guard.options_from_env() is None and not guard.enabled_from_env()
    monkeypatch.setenv("FASTVLA_STEP_GUARD_GROWTH_INTERVAL", "50")
    assert guard.options_from_env() is None                                  # the twins alone switch nothing on
    monkeypatch.setenv("FASTVLA_STEP_GUARD", "1")
    monkeypatch.setenv("FASTVLA_STEP_GUARD_DYNAMIC_LOSS_SCALE", "off")
    monkeypatch.setenv("FASTVLA_STEP_GUARD_MAX_LOSS_SCALE_LOG2", "16")
    assert guard.options_from_env() == dict(guard.DEFAULTS, growth_interval=50, dynamic_loss_scale=False, max_loss_scale_log2=16)
    got = guard.resolve_options(growth_interval=9, dynamic_loss_scale=True)
    assert got["growth_interval"] == 9 and got["dynamic_loss_scale"] is True and got["max_loss_scale_log2"] == 16
    monkeypatch.setenv("FASTVLA_STEP_GUARD_BACKOFF_LOG2", "half")
    with pytest.raises(ValueError, match="FASTVLA_STEP_GUARD_BACKOFF_LOG2"):
        guard.options_from_env()
    monkeypatch.delenv("FASTVLA_STEP_GUARD_BACKOFF_LOG2")
    monkeypatch.setenv("FASTVLA_STEP_GUARD", "maybe")
    with pytest.raises(ValueError, match="FASTVLA_STEP_GUARD "):
        guard.enabled_from_env()


def _policy():
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny", hidden_dim=16, fusion_dim=16))


def test_policy_options_are_resolved_and_refused_before_any_engine(monkeypatch):
    pol = _policy()
    assert not pol.step_guard_enabled and pol.step_guard_record() is None
    with pytest.raises(RuntimeError, match="step guard is off"):
        pol.step_guard_stats()
    with pytest.raises(ValueError) as ei:
        pol.enable_step_guard(min_loss_scale_log2=20, max_loss_scale_log2=8)
    assert "min_loss_scale_log2=20" in str(ei.value) and "max_loss_scale_log2=8" in str(ei.value) and not pol.step_guard_enabled
    opts = pol.enable_step_guard(dynamic_loss_scale=False, growth_interval=10)
    assert opts == dict(guard.DEFAULTS, dynamic_loss_scale=False, growth_interval=10) and pol.step_guard_enabled
    assert pol.enable_step_guard(dynamic_loss_scale=False, growth_interval=10) == opts          # the same options again: the running guard stays
    with pytest.raises(RuntimeError, match="already running"):
        pol.enable_step_guard(growth_interval=11)
    st = pol.step_guard_stats()                                              # before the first step: the initial state, no engine needed
    assert (st["delta_log2"], st["applied"], st["skipped_nonfinite"], st["loss_scale_log2"]) == (0, 0, 0, 0)
    pol.disable_step_guard()
    assert not pol.step_guard_enabled
    monkeypatch.setenv("FASTVLA_STEP_GUARD", "1")
    pol._step_guard_from_env()
    assert not pol.step_guard_enabled                                        # disable_step_guard() outlives the twin
    other = _policy()
    monkeypatch.setenv("FASTVLA_STEP_GUARD_GROWTH_LOG2", "2")
    other._step_guard_from_env()
    assert other.step_guard_enabled and other._sg["options"]["growth_log2"] == 2


def test_optimizer_record_key_only_when_the_guard_is_on():
    from vla_fastvlm.fastvla.guard_state import check_resume_step_guard
    from vla_fastvlm.utils.checkpoint import optimizer_record
    st = {"m": torch.zeros(4), "v": torch.zeros(4), "step": 3}
    plain = optimizer_record(st, None, 5, 3)
    assert "step_guard" not in plain and sorted(optimizer_record(st, None, 5, 3, step_guard=None)) == sorted(plain)
    pol = _policy()
    assert pol.step_guard_record() is None
    pol.enable_step_guard(growth_interval=5)
    rec = pol.step_guard_record()
    assert rec == {"options": dict(guard.DEFAULTS, growth_interval=5), "state": None}
    with_guard = optimizer_record(st, None, 5, 3, step_guard=rec)
    assert sorted(set(with_guard) - set(plain)) == ["step_guard"] and with_guard["step_guard"] == rec
    # a resume compares the options and names both; a record into a run without the guard is dropped with a warning
    check_resume_step_guard(rec["options"], pol._sg["options"])
    with pytest.raises(ValueError) as ei:
        check_resume_step_guard(dict(rec["options"], growth_interval=6), pol._sg["options"])
    assert "'growth_interval': 6" in str(ei.value) and "'growth_interval': 5" in str(ei.value)
    state = GuardRef(init_delta_log2=-1, min_delta_log2=-12, max_delta_log2=12).as_export()
    pol.load_step_guard_record({"options": rec["options"], "state": state})
    assert pol.step_guard_record()["state"] == state and pol.step_guard_stats()["delta_log2"] == -1
    off = _policy()
    with pytest.warns(UserWarning, match="guard off"):
        off.load_step_guard_record({"options": rec["options"], "state": state})
    assert not off.step_guard_enabled
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off.load_step_guard_record(None)


# ------------------------------------------------------------------------------------------------ the flag's exchange
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _flag_worker(rank, world, port, out):
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    for p_ in (str(root), str(root / "vla-from-fastvlm_amd"), str(root / "tests")):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    from fastvla_hip.guard import all_reduce_flag
    from step_guard_util import GuardRef
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    ref = GuardRef(init_delta_log2=0, min_delta_log2=-4, max_delta_log2=4, growth_interval=100)
    decisions = []
    for counter in (5, 5):                 # step 1: rank 0's backward saturated (its counter moved); step 2: nobody's did
        ref.observe(counter if rank == 0 else 0)
        flag = torch.tensor([float(ref.flag)])
        all_reduce_flag(flag)              # product code: SUM across the ranks
        ref.set_flag(int(flag[0]))
        decisions.append((float(flag[0]), ref.step(1.0), ref.delta_log2))
    out[rank] = decisions
    dist.destroy_process_group()


def test_one_flagged_rank_makes_both_ranks_skip():
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_flag_worker, args=(2, port, out), nprocs=2, join=True)
    assert out[0][0] == out[1][0] == (1.0, False, -1)       # one rank flagged: both saw the sum, both skipped, both halved
    assert out[0][1][1:] == out[1][1][1:] == (True, -1)     # the next step is applied on both


def test_single_process_flag_exchange_is_a_noop():
    flag = torch.tensor([1.0])
    guard.all_reduce_flag(flag)
    assert float(flag) == 1.0


def test_structs_match_the_header_layout():
    import ctypes as C
    from fastvla_hip import _lib
    assert C.sizeof(_lib.StepGuardConfig) == 32 and C.sizeof(_lib.StepGuardState) == 56
    assert [f[0] for f in _lib.StepGuardState._fields_] == list(guard.STATE_KEYS)
