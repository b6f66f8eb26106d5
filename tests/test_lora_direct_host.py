"""CPU: the host side of the direct LoRA backward -- the FASTVLA_LORA_DIRECT twin, the adapter config that stays free of the run's mode, and the refusals that
must come before a device is touched (the GPU side: tests/test_gpu_lora_direct.py)."""
import pytest

from fastvla_hip import _lib, lora


def test_direct_from_env():
    assert lora.direct_from_env({}) is False
    assert lora.direct_from_env({"FASTVLA_LORA_DIRECT": ""}) is False
    assert lora.direct_from_env({"FASTVLA_LORA_DIRECT": "0"}) is False
    assert lora.direct_from_env({"FASTVLA_LORA_DIRECT": "1"}) is True
    assert lora.direct_from_env({"FASTVLA_LORA_DIRECT": " 1 "}) is True
    for bad in ("yes", "true", "2", "-1", "on"):
        with pytest.raises(ValueError):
            lora.direct_from_env({"FASTVLA_LORA_DIRECT": bad})


def test_the_flag_stays_out_of_the_adapter_config():
    """the dict that adapter files, optimizer.pt and enable_backbone_training compare has exactly three keys, whatever FASTVLA_LORA_DIRECT says"""
    env = {"FASTVLA_LORA_RANK": "8", "FASTVLA_LORA_ALPHA": "16", "FASTVLA_LORA_TARGETS": "q,v", "FASTVLA_LORA_DIRECT": "1"}
    assert lora.config_from_env(env) == {"rank": 8, "alpha": 16.0, "targets": ["q_proj", "v_proj"]}
    assert lora.config_from_env({"FASTVLA_LORA_DIRECT": "1"}) is None
    assert set(lora.check_config(8)) == {"rank", "alpha", "targets"}


def test_entry_point_is_bound():
    assert "fv_train_lora_forward_backward" in _lib.SIGNATURES and len(_lib.SIGNATURES["fv_train_lora_forward_backward"][1]) == 20
    assert "fv_op_lora_direct" in _lib.OPS_SIGNATURES and "fv_op_lora_direct" not in _lib.SIGNATURES       # the kernels' op-level entry is test-only


def test_policy_refuses_direct_without_rank_before_it_touches_a_device(monkeypatch):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    for k in ("FASTVLA_LORA_RANK", "FASTVLA_LORA_ALPHA", "FASTVLA_LORA_TARGETS", "FASTVLA_LORA_DIRECT", "FASTVLA_TRAIN_TOWER"):
        monkeypatch.delenv(k, raising=False)
    pol = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:5", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False))
    with pytest.raises(ValueError):
        pol.enable_backbone_training(lora_direct=True)                               # no rank
    with pytest.raises(ValueError):
        pol.enable_backbone_training(tower=True, lora_direct=True)                   # no rank, and a trained tower
    with pytest.raises(ValueError):
        pol.enable_backbone_training(tower=True, lora_rank=8, lora_direct=True)      # adapters go with a frozen tower, in either backward mode
    monkeypatch.setenv("FASTVLA_LORA_DIRECT", "1")
    with pytest.raises(ValueError):
        pol.enable_backbone_training()                                               # the environment twin without FASTVLA_LORA_RANK
    monkeypatch.setenv("FASTVLA_LORA_DIRECT", "maybe")
    monkeypatch.setenv("FASTVLA_LORA_RANK", "8")
    monkeypatch.setenv("FASTVLA_TRAIN_TOWER", "1")
    with pytest.raises(ValueError):
        pol.enable_backbone_training()
    assert pol._unfrozen is None
