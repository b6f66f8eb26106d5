"""CPU: the host side of the DoRA / rsLoRA variants of LoRA mode -- configuration and environment parsing (the keys exist only when true: a plain run's
configuration is what it always was), the scale, the lora_layout(dora=True) mirror, the bindings, and the refusals that must come before a device is touched
(the GPU side: tests/test_gpu_dora.py)."""
import math

import pytest

from fastvla_hip import _lib, arch, lora


def test_config_keys_exist_only_when_true():
    assert lora.check_config(8) == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS)}
    assert lora.check_config(8, dora=False, rslora=False) == lora.check_config(8)
    assert set(lora.check_config(8)) == {"rank", "alpha", "targets"}
    assert lora.check_config(8, dora=True) == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS), "dora": True}
    assert lora.check_config(8, 16, "q,v", rslora=True) == {"rank": 8, "alpha": 16.0, "targets": ["q_proj", "v_proj"], "rslora": True}
    assert lora.check_config(8, dora=True, rslora=True) == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS), "dora": True, "rslora": True}
    for bad in ("yes", 2, 0.5):
        with pytest.raises(ValueError):
            lora.check_config(8, dora=bad)
        with pytest.raises(ValueError):
            lora.check_config(8, rslora=bad)
    with pytest.raises(ValueError):
        lora.check_config(8, tower=True, dora=True)          # adapters of any kind go with a frozen tower
    assert lora.variants_of(None) == {} and lora.variants_of(lora.check_config(8)) == {}
    assert lora.variants_of({"rank": 8, "alpha": 8.0, "targets": [], "dora": True}) == {"dora": True}
    assert lora.flags_of(lora.check_config(8)) == 0 and lora.flags_of(lora.check_config(8, dora=True)) == 1
    assert lora.flags_of(lora.check_config(8, rslora=True)) == 2 and lora.flags_of(lora.check_config(8, dora=True, rslora=True)) == 3


def test_scale_under_rslora():
    assert lora.scale_of(lora.check_config(16, 32.0)) == 2.0
    assert lora.scale_of(lora.check_config(16, 32.0, rslora=True)) == 8.0             # 32 / sqrt(16)
    assert lora.scale_of(lora.check_config(8, dora=True)) == 1.0                       # DoRA alone leaves the scale alone
    assert lora.scale_of(lora.check_config(7, 3.0, rslora=True)) == pytest.approx(3.0 / math.sqrt(7.0), rel=1e-15)
    assert lora.scale_of({"rank": 4, "alpha": 8.0, "targets": []}) == 2.0              # a record that predates the keys is plain LoRA


def test_environment_twins():
    base = {"FASTVLA_LORA_RANK": "8", "FASTVLA_LORA_ALPHA": "16", "FASTVLA_LORA_TARGETS": "q,v"}
    plain = {"rank": 8, "alpha": 16.0, "targets": ["q_proj", "v_proj"]}
    assert lora.config_from_env(base) == plain
    for off in ("", "0", " 0 "):
        assert lora.config_from_env({**base, "FASTVLA_LORA_DORA": off, "FASTVLA_LORA_RSLORA": off}) == plain
    assert lora.config_from_env({**base, "FASTVLA_LORA_DORA": "1"}) == {**plain, "dora": True}
    assert lora.config_from_env({**base, "FASTVLA_LORA_RSLORA": " 1 "}) == {**plain, "rslora": True}
    assert lora.config_from_env({**base, "FASTVLA_LORA_DORA": "1", "FASTVLA_LORA_RSLORA": "1"}) == {**plain, "dora": True, "rslora": True}
    for name in ("FASTVLA_LORA_DORA", "FASTVLA_LORA_RSLORA"):
        for bad in ("yes", "true", "2", "-1", "on"):
            with pytest.raises(ValueError):
                lora.config_from_env({**base, name: bad})
            with pytest.raises(ValueError):
                lora.variants_from_env({name: bad})
        with pytest.raises(ValueError):
            lora.config_from_env({name: "1"})                          # a variant without a rank
        with pytest.raises(ValueError):
            lora.config_from_env({name: "1", "FASTVLA_LORA_RANK": "0"})
        assert lora.config_from_env({name: "0"}) is None
    assert lora.variants_from_env({}) == {} and lora.variants_from_env({"FASTVLA_LORA_DORA": "1"}) == {"dora": True}


@pytest.mark.parametrize("targets", [None, ("q_proj", "v_proj", "down_proj")])
def test_layout_mirror_with_magnitudes(targets):
    model = arch.preset("small")
    rank = 6
    plain, ptotal = lora.lora_layout(model, rank, targets, hidden_dim=64, fusion_dim=64)
    dora, dtotal = lora.lora_layout(model, rank, targets, hidden_dim=64, fusion_dim=64, dora=True)
    assert lora.lora_layout(model, rank, targets, hidden_dim=64, fusion_dim=64, dora=False) == (plain, ptotal)
    assert dora[:16] == plain[:16] and dora[15]["name"] == "model.mm_projector.2.bias"          # head and projector keep their offsets
    assert dora[16]["offset"] == plain[16]["offset"] and dora[16]["name"].endswith(".lora_A.weight")
    names = lora.parse_targets(targets)
    shp = lora.logical_shapes(model)
    assert len(dora) == 16 + 3 * len(names) * model.llm.layers and len(plain) == 16 + 2 * len(names) * model.llm.layers
    off = dora[16]["offset"]
    extra = 0
    for n, t in enumerate(dora[16:]):
        layer, tgt = n // (3 * len(names)), names[n // 3 % len(names)]
        out_, in_ = shp[tgt]
        kind = n % 3
        pre = f"model.layers.{layer}.{'self_attn' if tgt[0] in 'qkvo' else 'mlp'}.{tgt}"
        want = [(pre + ".lora_A.weight", rank, in_), (pre + ".lora_B.weight", out_, rank), (pre + ".lora_magnitude_vector.weight", 1, out_)][kind]
        assert (t["name"], t["rows"], t["cols"]) == want and t["numel"] == want[1] * want[2] and t["bucket"] == 3 + layer and t["packing"] == 0
        assert t["offset"] == off and off % 4 == 0                        # every tensor on a multiple of 4 floats, nothing between them but that padding
        off += (t["numel"] + 3) // 4 * 4
        if kind == 2:
            extra += (t["numel"] + 3) // 4 * 4
    assert off == dtotal == ptotal + extra
    # the adapters themselves are the plain layout's, in its order
    assert [(t["name"], t["numel"]) for t in dora if ".lora_magnitude_vector." not in t["name"]] == [(t["name"], t["numel"]) for t in plain]


def test_layout_pads_a_magnitude_that_is_no_multiple_of_four():
    llm = arch.LLMConfig(hidden=96, layers=1, heads=3, kv_heads=1, head_dim=32, inter=160, vocab=64)       # kv rows 32, hidden 96; rank 5: odd A / B sizes
    model = arch.ModelConfig("odd", llm, arch.preset("tiny").tower)
    t, total = lora.lora_layout(model, 5, ("k_proj",), hidden_dim=64, fusion_dim=64, dora=True)
    a, b, m = t[16:]
    assert (a["numel"], b["numel"], m["numel"]) == (5 * 96, 32 * 5, 32)
    assert b["offset"] == a["offset"] + 480 and m["offset"] == b["offset"] + 160 and total == m["offset"] + 32


def test_entry_points_are_bound():
    assert _lib.SIGNATURES["fv_train_lora_begin_ex"][1] == _lib.SIGNATURES["fv_train_lora_begin"][1] + [_lib.SIGNATURES["fv_train_lora_begin"][1][1]]
    assert len(_lib.SIGNATURES["fv_train_lora_init_magnitude"][1]) == 4
    assert len(_lib.SIGNATURES["fv_train_lora_commit"][1]) == 4 and len(_lib.SIGNATURES["fv_train_lora_project"][1]) == 5      # the old entry points keep their signatures
    assert (lora.FLAG_DORA, lora.FLAG_RSLORA) == (1, 2)


def _policy():
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:5", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False))


ENV_KEYS = ("FASTVLA_LORA_RANK", "FASTVLA_LORA_ALPHA", "FASTVLA_LORA_TARGETS", "FASTVLA_LORA_DIRECT", "FASTVLA_LORA_DORA", "FASTVLA_LORA_RSLORA", "FASTVLA_TRAIN_TOWER")


def test_policy_refuses_dora_with_direct_before_it_touches_a_device(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    pol = _policy()
    with pytest.raises(ValueError) as e:
        pol.enable_backbone_training(lora_rank=8, lora_dora=True, lora_direct=True)
    assert "lora_dora" in str(e.value) and "lora_direct" in str(e.value)                 # the message names both
    monkeypatch.setenv("FASTVLA_LORA_DIRECT", "1")
    with pytest.raises(ValueError) as e:
        pol.enable_backbone_training(lora_rank=8, lora_dora=True)                        # ... the environment twin of either
    assert "lora_dora" in str(e.value) and "lora_direct" in str(e.value)
    monkeypatch.delenv("FASTVLA_LORA_DIRECT")
    monkeypatch.setenv("FASTVLA_LORA_DORA", "1")
    with pytest.raises(ValueError):
        pol.enable_backbone_training(lora_rank=8, lora_direct=True)
    with pytest.raises(ValueError):
        pol.enable_backbone_training()                                                   # FASTVLA_LORA_DORA without a rank
    monkeypatch.setenv("FASTVLA_LORA_DORA", "maybe")
    with pytest.raises(ValueError):
        pol.enable_backbone_training(lora_rank=8)
    monkeypatch.delenv("FASTVLA_LORA_DORA")
    for kw in ({"lora_dora": True}, {"lora_rslora": True}):
        with pytest.raises(ValueError):
            pol.enable_backbone_training(**kw)                                           # a variant without a rank
    with pytest.raises(ValueError):
        pol.enable_backbone_training(tower=True, lora_rank=8, lora_dora=True)
    assert pol._unfrozen is None


class _FakeState:
    """UnfrozenState.load_lora_state's configuration check alone: it compares before it reads a tensor or touches the engine"""

    def __init__(self, cfg):
        self.lora = cfg
        self.lora_tensors = []
        self.lora_adapters_zero = True
        self.commits = 0

    def commit(self):
        self.commits += 1


def test_adapter_file_config_mismatch_names_both_configs():
    from vla_fastvlm.training.unfrozen import UnfrozenState
    plain, dora, rs = lora.check_config(8), lora.check_config(8, dora=True), lora.check_config(8, rslora=True)
    for run, file in ((plain, dora), (dora, plain), (plain, rs), (rs, plain), (dora, rs), (dora, lora.check_config(8, dora=True, rslora=True))):
        with pytest.raises(ValueError) as e:
            UnfrozenState.load_lora_state(_FakeState(run), {"config": dict(file), "tensors": {}})
        assert str(file) in str(e.value) and str(run) in str(e.value)
    # an old file (no variant keys) is plain LoRA: a plain run takes it -- nothing raises, the (empty) tensor list is loaded and the state commits
    old = _FakeState(plain)
    UnfrozenState.load_lora_state(old, {"config": {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS)}, "tensors": {}})
    assert old.commits == 1 and old.lora_adapters_zero is False
    # ... and a file that spells the variants out as false is the same plain file
    UnfrozenState.load_lora_state(old, {"config": {**plain, "dora": False, "rslora": False}, "tensors": {}})
    assert old.commits == 2
