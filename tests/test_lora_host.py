"""CPU: the host side of the LoRA mode of backbone training (fastvla_hip/lora.py, FastVLAPolicy.enable_backbone_training(lora_rank=...)): the trainable
buffer's layout against PEFT's key names written out by hand, the argument refusals, the environment twins, and the data-parallel exchange of the trainable
buffer over gloo.  (tests/test_gpu_lora.py holds the library's fv_train_lora_layout to the same layout function on the device.)"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fastvla_hip import arch, lora

# (hidden, layers, q rows, kv rows, inter) written out from the model cards, not computed from the presets
GEOMETRY = {"fastvlm-0.5b": (896, 24, 896, 128, 4864), "fastvlm-1.5b": (1536, 28, 1536, 256, 8960), "fastvlm-7b": (3584, 28, 3584, 512, 18944)}
HEAD = ["state_projection.0.weight", "state_projection.0.bias", "state_projection.1.weight", "state_projection.1.bias", "fusion.0.weight", "fusion.0.bias",
        "fusion.1.weight", "fusion.1.bias", "fusion.4.weight", "fusion.4.bias", "action_head.weight", "action_head.bias"]
PROJECTOR = ["model.mm_projector.0.weight", "model.mm_projector.0.bias", "model.mm_projector.2.weight", "model.mm_projector.2.bias"]


def _peft_keys(l, H, Q, KV, I, r):
    """PEFT's state-dict keys of one Qwen2 decoder layer with all seven projections adapted, in module order, with their shapes"""
    p = f"model.layers.{l}."
    return [(p + "self_attn.q_proj.lora_A.weight", (r, H)), (p + "self_attn.q_proj.lora_B.weight", (Q, r)),
            (p + "self_attn.k_proj.lora_A.weight", (r, H)), (p + "self_attn.k_proj.lora_B.weight", (KV, r)),
            (p + "self_attn.v_proj.lora_A.weight", (r, H)), (p + "self_attn.v_proj.lora_B.weight", (KV, r)),
            (p + "self_attn.o_proj.lora_A.weight", (r, Q)), (p + "self_attn.o_proj.lora_B.weight", (H, r)),
            (p + "mlp.gate_proj.lora_A.weight", (r, H)), (p + "mlp.gate_proj.lora_B.weight", (I, r)),
            (p + "mlp.up_proj.lora_A.weight", (r, H)), (p + "mlp.up_proj.lora_B.weight", (I, r)),
            (p + "mlp.down_proj.lora_A.weight", (r, I)), (p + "mlp.down_proj.lora_B.weight", (H, r))]


@pytest.mark.parametrize("name", sorted(GEOMETRY))
@pytest.mark.parametrize("rank", [4, 16, 64])
def test_layout_names_and_shapes_are_pefts(name, rank):
    H, L, Q, KV, I = GEOMETRY[name]
    model = arch.preset(name)
    tensors, total = lora.lora_layout(model, rank)
    assert [t["name"] for t in tensors[:16]] == HEAD + PROJECTOR
    assert [t["bucket"] for t in tensors[:16]] == [0] * 12 + [1] * 4
    assert (tensors[12]["rows"], tensors[12]["cols"]) == (H, model.tower.out_dim) and (tensors[14]["rows"], tensors[14]["cols"]) == (H, H)
    want = [kv for l in range(L) for kv in _peft_keys(l, H, Q, KV, I, rank)]
    got = [(t["name"], (t["rows"], t["cols"])) for t in tensors[16:]]
    assert got == want
    assert all(t["packing"] == 0 and t["numel"] == t["rows"] * t["cols"] and t["offset"] % 4 == 0 for t in tensors)
    assert all(a["offset"] + (a["numel"] + 3) // 4 * 4 == b["offset"] for a, b in zip(tensors, tensors[1:]))     # contiguous, 16-byte aligned
    assert total == tensors[-1]["offset"] + (tensors[-1]["numel"] + 3) // 4 * 4
    assert [t["bucket"] for t in tensors[16:]] == [3 + l for l in range(L) for _ in range(14)]
    adapters = sum(t["numel"] for t in tensors[16:])
    assert adapters == L * rank * ((H + Q) + 2 * (H + KV) + (Q + H) + 2 * (H + I) + (I + H))
    # the point of the mode: a fraction of the decoder's own matrices
    assert adapters < 0.1 * L * (H * (Q + 2 * KV) + Q * H + 3 * H * I)


def test_targets_subset_and_order():
    model = arch.preset("fastvlm-0.5b")
    tensors, _ = lora.lora_layout(model, 4, ["v_proj", "q"])
    names = [t["name"] for t in tensors[16:30]]
    assert names[:4] == ["model.layers.0.self_attn.q_proj.lora_A.weight", "model.layers.0.self_attn.q_proj.lora_B.weight",
                         "model.layers.0.self_attn.v_proj.lora_A.weight", "model.layers.0.self_attn.v_proj.lora_B.weight"]
    assert len(tensors) == 16 + 4 * 24 and not any("k_proj" in t["name"] or "mlp" in t["name"] for t in tensors)
    assert lora.parse_targets("q_proj, down_proj") == ("q_proj", "down_proj") and lora.parse_targets("all") == lora.TARGETS == lora.parse_targets(None)
    assert lora.target_mask(None) == 127 and lora.target_mask(["q_proj", "v_proj"]) == 5 and lora.targets_of_mask(5) == ("q_proj", "v_proj")


def test_argument_refusals():
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError):
            lora.check_config(bad)
    with pytest.raises(ValueError, match="unknown LoRA target"):
        lora.check_config(8, targets=["q_proj", "lm_head"])
    with pytest.raises(ValueError):
        lora.check_config(8, targets=[])
    with pytest.raises(ValueError):
        lora.check_config(8, alpha=0.0)
    with pytest.raises(ValueError, match="tower"):
        lora.check_config(8, tower=True)
    assert lora.check_config(8) == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS)}          # defaults: alpha = rank, all seven
    assert lora.check_config(64, 16, "q,v") == {"rank": 64, "alpha": 16.0, "targets": ["q_proj", "v_proj"]}


def test_policy_refuses_before_it_touches_a_device(monkeypatch):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    for k in ("FASTVLA_LORA_RANK", "FASTVLA_LORA_ALPHA", "FASTVLA_LORA_TARGETS", "FASTVLA_TRAIN_TOWER"):
        monkeypatch.delenv(k, raising=False)
    pol = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:small:41", hidden_dim=64, fusion_dim=64, freeze_backbone=False))
    with pytest.raises(ValueError, match="tower"):
        pol.enable_backbone_training(tower=True, lora_rank=8)
    for kw in (dict(lora_rank=0), dict(lora_rank=65), dict(lora_rank=8, lora_targets=["nope"]), dict(lora_alpha=4.0), dict(lora_targets=["q_proj"])):
        with pytest.raises(ValueError):
            pol.enable_backbone_training(**kw)
    with pytest.raises(RuntimeError, match="no LoRA adapters"):
        pol.merge_lora()
    monkeypatch.setenv("FASTVLA_LORA_RANK", "8")
    monkeypatch.setenv("FASTVLA_TRAIN_TOWER", "1")
    with pytest.raises(ValueError, match="tower"):
        pol.enable_backbone_training()
    assert pol._unfrozen is None


def test_environment_twins():
    assert lora.config_from_env({}) is None and lora.config_from_env({"FASTVLA_LORA_RANK": "0"}) is None and lora.config_from_env({"FASTVLA_LORA_RANK": ""}) is None
    assert lora.config_from_env({"FASTVLA_LORA_RANK": "16"}) == {"rank": 16, "alpha": 16.0, "targets": list(lora.TARGETS)}
    assert lora.config_from_env({"FASTVLA_LORA_RANK": "16", "FASTVLA_LORA_ALPHA": "32", "FASTVLA_LORA_TARGETS": "q_proj,v_proj"}) == \
        {"rank": 16, "alpha": 32.0, "targets": ["q_proj", "v_proj"]}
    for bad in ({"FASTVLA_LORA_RANK": "65"}, {"FASTVLA_LORA_RANK": "x"}, {"FASTVLA_LORA_RANK": "8", "FASTVLA_LORA_TARGETS": "q_proj,wte"}):
        with pytest.raises(ValueError):
            lora.config_from_env(bad)


def test_adapter_initialisation_is_pefts():
    model = arch.preset("small")
    tensors, total = lora.lora_layout(model, 8, hidden_dim=64, fusion_dim=64)
    flat = torch.full((total,), 7.0)
    lora.init_adapters(flat, tensors, seed=3)
    again = torch.full((total,), 7.0)
    lora.init_adapters(again, tensors, seed=3)
    assert torch.equal(flat, again)                                    # seeded
    front = tensors[16]["offset"]
    assert float((flat[:front] - 7.0).abs().max()) == 0.0              # head and projector are not touched
    for name, v in lora.adapter_views(flat, tensors).items():
        if name.endswith("lora_B.weight"):
            assert float(v.abs().max()) == 0.0
        else:   # kaiming_uniform_(a = sqrt(5)) on an (r, in) matrix: U(-1/sqrt(in), 1/sqrt(in))
            bound = v.shape[1] ** -0.5
            assert float(v.abs().max()) <= bound and abs(float(v.std()) - bound / 3 ** 0.5) < 0.15 * bound


# ---------------------------------------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _mini():
    """a miniature decoder layer set: the trainable buffer of the `small` preset at rank 4, q and v only"""
    model = arch.preset("small")
    tensors, total = lora.lora_layout(model, 4, ["q_proj", "v_proj"], hidden_dim=16, fusion_dim=16)
    g = torch.Generator().manual_seed(2)
    params = torch.randn(total, generator=g) * 0.1
    shapes = lora.logical_shapes(model)
    return model, tensors, total, params, shapes


def _project(tensors, params, dW, s, out):
    """dA = s B^T dW, dB = s dW A^T on the CPU, into the trainable layout; head / projector slots take dW['front']"""
    front = tensors[16]["offset"]
    out[:front] = dW["front"]
    par, dst = lora.adapter_views(params, tensors), lora.adapter_views(out, tensors)
    for name in par:
        if name.endswith(".lora_A.weight"):
            nb = name.replace(".lora_A.", ".lora_B.")
            d = dW[name.replace(".lora_A.weight", ".weight")]
            dst[name].copy_(s * par[nb].t() @ d)
            dst[nb].copy_(s * d @ par[name].t())


def _rank_grads(model, tensors, shapes, rank_id):
    g = torch.Generator().manual_seed(100 + rank_id)
    dW = {"front": torch.randn(tensors[16]["offset"], generator=g)}
    for l in range(model.llm.layers):
        for t in ("q_proj", "v_proj"):
            dW[f"model.layers.{l}.self_attn.{t}.weight"] = torch.randn(*shapes[t], generator=g)
    return dW


def _worker(rank, world, port, out):
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    for p_ in (str(root), str(root / "vla-from-fastvlm_amd")):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    from vla_fastvlm.training.dp import GradExchange
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    model, tensors, total, params, shapes = _mini()
    lg = torch.zeros(total)
    _project(tensors, params, _rank_grads(model, tensors, shapes, rank), 2.0, lg)
    ex = GradExchange(None)                         # product code: ONE all-reduce (sum) of the trainable buffer, returns 1 / world
    scale = ex.start(lg)
    ex.finish()
    out[rank] = ((lg * scale).clone(), ex.last_numel)
    dist.destroy_process_group()


def test_two_rank_exchange_of_the_trainable_buffer_equals_the_full_batch_projection():
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    model, tensors, total, params, shapes = _mini()
    (g0, n0), (g1, n1) = out[0], out[1]
    assert n0 == n1 == total                        # the payload is the trainable numel -- not the decoder's
    decoder = model.llm.layers * sum(a * b for a, b in shapes.values())
    assert total < 0.5 * decoder
    assert torch.equal(g0, g1)
    # projecting is linear: the mean of the ranks' projected gradients is the projection of the full batch's (mean) dW
    d0, d1 = _rank_grads(model, tensors, shapes, 0), _rank_grads(model, tensors, shapes, 1)
    ref = torch.zeros(total)
    _project(tensors, params, {k: 0.5 * (d0[k] + d1[k]) for k in d0}, 2.0, ref)
    assert float((g0 - ref).norm() / ref.norm()) <= 1e-6
