"""CPU: the host side of the parameter groups of the fused clip + AdamW step -- fastvla_hip/optim.py (options, environment twins, the group table of a
layout), the fv_adamw_group struct, and the optimizer.pt record.  No device call is made."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from fastvla_hip import _lib, arch, lora, optim


def _tiles(groups, total):
    assert groups[0]["begin"] == 0 and groups[-1]["end"] == total
    assert all(a["end"] == b["begin"] for a, b in zip(groups, groups[1:]))
    assert all(g["begin"] % 4 == 0 and g["end"] % 4 == 0 and g["end"] > g["begin"] for g in groups)
    # merging: no two neighbours carry the same settings
    key = lambda g: (g["lr_scale"], g["weight_decay"], g["frozen"])  # noqa: E731
    assert all(key(a) != key(b) for a, b in zip(groups, groups[1:]))


def _group_of(groups, t):
    return next(g for g in groups if g["begin"] <= t["offset"] < g["end"])


def _full_layout(L=3, tower=True):
    """a hand-made fv_train_layout: head (two tensors), projector, embedding, L layers of [norm, matrix, bias], the final norm, two tower tensors; odd sizes, so
    that most tensors carry padding"""
    out, off = [], 0

    def add(name, rows, cols, bucket):
        nonlocal off
        out.append(dict(name=name, offset=off, numel=rows * cols, rows=rows, cols=cols, bucket=bucket, packing=0))
        off += (rows * cols + 3) // 4 * 4

    add("state_projection.0.weight", 1, 14, 0)
    add("action_head.weight", 14, 9, 0)
    add("model.mm_projector.0.weight", 6, 7, 1)
    add("model.mm_projector.0.bias", 1, 6, 1)
    add("model.embed_tokens.weight", 11, 6, 2)
    for l in range(L):
        add(f"model.layers.{l}.input_layernorm.weight", 1, 6, 3 + l)
        add(f"model.layers.{l}.self_attn.qkv_proj.weight", 10, 6, 3 + l)
        add(f"model.layers.{l}.self_attn.qkv_proj.bias", 1, 10, 3 + l)
    add("model.norm.weight", 1, 6, 3 + L)
    if tower:
        add("model.vision_tower.vision_tower.model.patch_embed.0.reparam_conv.weight", 27, 5, 3 + L + 1)
        add("model.vision_tower.vision_tower.model.network.0.0.layer_scale", 1, 5, 3 + L + 2)
    return out, off


def test_struct_and_segment_constant_match_the_header():
    assert C.sizeof(_lib.AdamWGroup) == 32 and C.sizeof(_lib.AdamWHParams) == 28
    assert [f[0] for f in _lib.AdamWGroup._fields_] == ["begin", "end", "lr_scale", "weight_decay", "frozen", "reserved"]
    assert _lib.AdamWGroup.lr_scale.offset == 16 and _lib.AdamWGroup.frozen.offset == 24
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "fastvla_hip.h").read_text()
    assert f"#define FV_ADAMW_SEGMENT {_lib.FV_ADAMW_SEGMENT}" in header and _lib.FV_ADAMW_SEGMENT == 8192


def test_no_option_is_one_group_over_the_whole_buffer():
    tensors, total = _full_layout()
    groups, names = optim.build_param_groups(tensors, weight_decay=1e-4)
    assert groups == [dict(begin=0, end=total, lr_scale=1.0, weight_decay=1e-4, frozen=False)] and len(names) == 1
    assert optim.normalize_options() == {} and optim.options_from_env({}) == {}


def test_full_layout_sections_factors_padding_and_merging():
    L = 3
    tensors, total = _full_layout(L)
    by = {t["name"]: t for t in tensors}
    assert optim.decoder_layers(tensors) == L
    assert [optim.section_of(t, L) for t in tensors[:5]] == ["head", "head", "projector", "projector", "embedding"]
    assert optim.section_of(by["model.norm.weight"], L) == "decoder" and optim.section_of(tensors[-1], L) == "tower"
    groups, names = optim.build_param_groups(tensors, weight_decay=0.01, lr_scales={"decoder": 0.1, "embedding": 0.5, "tower": 0.25}, no_decay=("vectors",),
                                             layer_decay=0.9, freeze=("embedding",))
    _tiles(groups, total)
    assert len(names) == len(groups)
    g = lambda n: _group_of(groups, by[n])  # noqa: E731
    # factor products: section x layer decay
    for l in range(L):
        w = g(f"model.layers.{l}.self_attn.qkv_proj.weight")
        assert w["lr_scale"] == pytest.approx(0.1 * 0.9 ** (L - 1 - l), rel=1e-12) and w["weight_decay"] == 0.01 and not w["frozen"]
        for v in (f"model.layers.{l}.input_layernorm.weight", f"model.layers.{l}.self_attn.qkv_proj.bias"):
            assert g(v)["lr_scale"] == w["lr_scale"] and g(v)["weight_decay"] == 0.0
    assert g("model.layers.2.self_attn.qkv_proj.weight")["lr_scale"] == pytest.approx(0.1)          # the last layer: d^0
    assert g("model.norm.weight")["lr_scale"] == pytest.approx(0.1) and g("model.norm.weight")["weight_decay"] == 0.0
    e = g("model.embed_tokens.weight")
    assert e["frozen"] and e["lr_scale"] == pytest.approx(0.5 * 0.9 ** L, rel=1e-12)
    assert g("state_projection.0.weight")["lr_scale"] == 1.0 and g("state_projection.0.weight")["weight_decay"] == 0.0       # a head vector
    assert g("action_head.weight")["lr_scale"] == 1.0 and g("action_head.weight")["weight_decay"] == 0.01
    assert g(tensors[-2]["name"])["lr_scale"] == 0.25 and g(tensors[-1]["name"]) == dict(g(tensors[-1]["name"]), lr_scale=0.25, weight_decay=0.0)
    # padding ownership: a tensor's group runs to the next tensor's offset (66 floats of embedding own the 2 behind them)
    assert e["begin"] == by["model.embed_tokens.weight"]["offset"] and e["end"] == by["model.layers.0.input_layernorm.weight"]["offset"] == e["begin"] + 68
    assert by["model.embed_tokens.weight"]["numel"] == 66
    # merging: layer l's bias and layer l + 1's norm differ (layer decay), but the last layer's bias and the final norm are one group
    last = g("model.layers.2.self_attn.qkv_proj.bias")
    assert last is g("model.norm.weight") and "2 tensors" in names[groups.index(last)]
    assert g("model.layers.0.self_attn.qkv_proj.bias") is not g("model.layers.1.input_layernorm.weight")
    # action_head.weight and mm_projector.0.weight: both plain matrices at factor 1 -> one group
    assert g("action_head.weight") is g("model.mm_projector.0.weight")
    # freezing the class: every vector, wherever it sits
    groups, _ = optim.build_param_groups(tensors, weight_decay=0.01, freeze=("vectors", "tower"))
    _tiles(groups, total)
    for t in tensors:
        assert _group_of(groups, t)["frozen"] == (t["rows"] == 1 or "vision_tower" in t["name"]), t["name"]
    # an explicit total extends the last group; one that cuts a tensor, or is not a multiple of 4, raises
    groups, _ = optim.build_param_groups(tensors, weight_decay=0.0, total=total + 8)
    assert groups[-1]["end"] == total + 8
    with pytest.raises(ValueError):
        optim.build_param_groups(tensors, weight_decay=0.0, total=total - 8)
    with pytest.raises(ValueError, match="multiples of 4"):
        optim.build_param_groups(tensors, weight_decay=0.0, total=total + 2)


def test_lora_layout_lora_plus_layer_decay_and_magnitudes():
    model = arch.preset("small")
    L = model.llm.layers
    tensors, total = lora.lora_layout(model, 4, None, hidden_dim=64, fusion_dim=64, dora=True)
    assert optim.decoder_layers(tensors) == L
    groups, names = optim.build_param_groups(tensors, weight_decay=0.3, lora_plus_ratio=16, no_decay=("vectors",), layer_decay=0.8, lr_scales={"adapters": 2.0})
    _tiles(groups, total)
    assert len(groups) > 7 * L          # "hundreds of groups" at 24 layers: A / B / magnitude alternate
    for t in tensors:
        g = _group_of(groups, t)
        if ".lora_" not in t["name"]:
            assert g["lr_scale"] == 1.0 and optim.section_of(t, L) in ("head", "projector")
            continue
        assert optim.section_of(t, L) == "adapters"
        base = 2.0 * 0.8 ** (L - 1 - (t["bucket"] - 3))
        if ".lora_B." in t["name"]:
            assert g["lr_scale"] == pytest.approx(16 * base, rel=1e-12) and g["weight_decay"] == 0.3
        elif ".lora_A." in t["name"]:
            assert g["lr_scale"] == pytest.approx(base, rel=1e-12) and g["weight_decay"] == 0.3
        else:
            assert t["rows"] == 1 and g["lr_scale"] == pytest.approx(base, rel=1e-12) and g["weight_decay"] == 0.0      # a magnitude is never decayed towards zero
    # without DoRA and without options that tell A from B, a layer's adapters are one group
    tensors, total = lora.lora_layout(model, 4, ["q_proj", "v_proj"], hidden_dim=64, fusion_dim=64)
    groups, names = optim.build_param_groups(tensors, weight_decay=0.3, layer_decay=0.5)
    _tiles(groups, total)
    assert [n for n in names if ".lora_" in n and "4 tensors" in n] and len([g for g in groups if g["lr_scale"] != 1.0]) == L - 1


def test_refusals():
    tensors, _ = _full_layout()
    with pytest.raises(ValueError, match="unknown section 'backbone'"):
        optim.build_param_groups(tensors, weight_decay=0.0, lr_scales={"backbone": 0.1})
    with pytest.raises(ValueError, match="unknown section"):
        optim.build_param_groups(tensors, weight_decay=0.0, lr_scales={"vectors": 0.1})      # the class is for no_decay / freeze only
    with pytest.raises(ValueError, match="unknown section"):
        optim.build_param_groups(tensors, weight_decay=0.0, no_decay=("norms",))
    with pytest.raises(ValueError, match="unknown section"):
        optim.build_param_groups(tensors, weight_decay=0.0, freeze="embedding,nothing")
    with pytest.raises(ValueError, match="lora_plus_ratio needs LoRA adapters"):
        optim.build_param_groups(tensors, weight_decay=0.0, lora_plus_ratio=16)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            optim.build_param_groups(tensors, weight_decay=0.0, lr_scales={"head": bad})
        with pytest.raises(ValueError):
            optim.build_param_groups(tensors, weight_decay=bad)
    with pytest.raises(ValueError):
        optim.build_param_groups(tensors, weight_decay=0.0, layer_decay=0.0)
    crooked = [dict(t) for t in tensors]
    crooked[3]["offset"] += 2
    with pytest.raises(ValueError, match="multiples of 4"):
        optim.build_param_groups(crooked, weight_decay=0.0)
    with pytest.raises(ValueError):
        optim.build_param_groups([], weight_decay=0.0)


def test_environment_twins():
    env = {"FASTVLA_LR_SCALES": "decoder=0.1, tower=0.1", "FASTVLA_NO_DECAY": "vectors", "FASTVLA_LAYER_DECAY": "0.9", "FASTVLA_LORA_PLUS_RATIO": "16",
           "FASTVLA_FREEZE": "embedding,vectors"}
    assert optim.options_from_env(env) == {"lr_scales": {"decoder": 0.1, "tower": 0.1}, "no_decay": ["vectors"], "layer_decay": 0.9, "lora_plus_ratio": 16.0,
                                           "freeze": ["embedding", "vectors"]}
    assert optim.options_from_env(env) == optim.normalize_options(lr_scales={"tower": 0.1, "decoder": 0.1}, no_decay=("vectors",), layer_decay=0.9, lora_plus_ratio=16,
                                                                  freeze=("vectors", "embedding"))
    assert optim.options_from_env({"FASTVLA_LR_SCALES": "", "FASTVLA_FREEZE": "  "}) == {}
    assert optim.options_from_env({"FASTVLA_NO_DECAY": "vectors"}) == {"no_decay": ["vectors"]}
    for bad in ({"FASTVLA_LR_SCALES": "decoder"}, {"FASTVLA_LR_SCALES": "decoder=x"}, {"FASTVLA_LR_SCALES": "llm=0.1"}, {"FASTVLA_LR_SCALES": "head=1,head=2"},
                {"FASTVLA_LAYER_DECAY": "fast"}, {"FASTVLA_LAYER_DECAY": "0"}, {"FASTVLA_LORA_PLUS_RATIO": "-2"}, {"FASTVLA_FREEZE": "everything"}):
        with pytest.raises(ValueError):
            optim.options_from_env(bad)
    # explicit_kwargs spells every list / dict option out, so that no twin can fill it in; normalising it again gives the options back
    o = optim.options_from_env(env)
    assert optim.normalize_options(**optim.explicit_kwargs(o)) == o
    assert optim.explicit_kwargs({}) == {"lr_scales": {}, "no_decay": (), "freeze": ()}


def test_checkpoint_record_carries_the_options_only_when_one_is_set():
    from vla_fastvlm.utils.checkpoint import check_resume_optim, optimizer_record
    st = {"m": torch.zeros(8), "v": torch.zeros(8), "step": 3}
    plain = SimpleNamespace(trainable=torch.zeros(8), train_tower=False, lora=None, optim={})
    rec = optimizer_record(st, plain, 5, 4)
    assert sorted(rec) == sorted(["m", "v", "step", "global_step", "update_step", "flat", "train_backbone", "train_tower"])       # a plain run's keys, as before
    assert sorted(optimizer_record(st, None, 5, 4)) == sorted(["m", "v", "step", "global_step", "update_step"])                   # head-only training
    opts = optim.normalize_options(no_decay=("vectors",), lora_plus_ratio=16)
    with_opts = SimpleNamespace(trainable=torch.zeros(8), train_tower=False, lora={"rank": 4, "alpha": 8.0, "targets": ["q_proj"]}, optim=opts)
    rec = optimizer_record(st, with_opts, 5, 4)
    assert rec["optim"] == opts and rec["optim"] is not opts and rec["lora"]["rank"] == 4
    check_resume_optim(None, {})
    check_resume_optim(opts, dict(opts))
    with pytest.raises(ValueError) as ei:
        check_resume_optim(opts, optim.normalize_options(lora_plus_ratio=4))
    assert "16.0" in str(ei.value) and "4.0" in str(ei.value)
    with pytest.raises(ValueError, match="this run uses none"):
        check_resume_optim(opts, {})
    with pytest.raises(ValueError, match="options none"):
        check_resume_optim({}, opts)
