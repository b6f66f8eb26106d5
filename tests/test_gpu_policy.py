"""-m gpu: the drop-in Python surface (vla_fastvlm.fastvla / lerobot_fastvla) driving the HIP path, against the oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, check_close, rel_l2  # noqa: E402
from fastvla_hip import HEAD_KEYS, arch, weights  # noqa: E402
from oracle import fastvit_hd, head, policy, qwen2  # noqa: E402
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy  # noqa: E402


def _oracle_cfgs(m):
    return (fastvit_hd.TowerCfg(layers=m.tower.layers, dims=m.tower.dims),
            qwen2.Qwen2Cfg(hidden=m.llm.hidden, layers=m.llm.layers, heads=m.llm.heads, kv_heads=m.llm.kv_heads,
                           head_dim=m.llm.head_dim, inter=m.llm.inter, vocab=m.llm.vocab))


@pytest.fixture(scope="module")
def pol():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    torch.manual_seed(21)
    p = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0))
    return p.to(DEV)


def _batch(B=3):
    g = torch.Generator().manual_seed(5)
    return {"images": torch.rand(B, 2, 3, 72, 96, generator=g), "states": torch.randn(B, 2, 14, generator=g),
            "actions": torch.randn(B, 14, generator=g), "tasks": ["stack the red block", "open drawer", "x"][:B]}


def _oracle_actions(pol, batch, head_p):
    m = arch.preset("tiny")
    tc, lc = _oracle_cfgs(m)
    w = weights.init_backbone(m, seed=77)
    tasks = policy.normalize_tasks(batch["tasks"], batch["images"].shape[0])
    tok = pol.model.backbone.tokenizer(tasks, padding="longest", truncation=True, max_length=64)
    pooled, _ = policy.backbone_features(w, policy.last_timestep(batch["images"], 4), tok["input_ids"], tok["attention_mask"],
                                         image_size=m.tower.image_size, llm_cfg=lc, tower_cfg=tc)
    return pooled, policy.last_timestep(batch["states"], 2)


def test_compute_loss_and_autograd_backward(pol):
    batch = _batch()
    pol.train()
    head_p = {k: v.detach().cpu().clone() for k, v in zip(HEAD_KEYS, pol.model.head_parameters())}
    out = pol.compute_loss({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()})
    out["loss"].backward()
    torch.cuda.synchronize()
    pooled, states = _oracle_actions(pol, batch, head_p)
    pred, cache = head.head_forward(head_p, pooled, states, keep_cache=True)
    loss, grads = head.head_mse_backward(head_p, cache, pred, batch["actions"])
    assert abs(float(out["loss"].detach()) - float(loss)) <= 1e-3 * float(loss)   # north_star's bar
    assert set(out) == {"loss", "mse"} and not out["mse"].requires_grad
    for k, p in zip(HEAD_KEYS, pol.model.head_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape
        assert rel_l2(p.grad.cpu(), grads[k]) <= 1e-3, k   # the same path measures ~1e-5 at full size (test_gpu_fullsize.py)
    fg = pol.model.flat_grads()  # autograd may keep the returned views (one flat buffer) or clone them
    print("grads stay views of one flat buffer:", fg is not None)
    # a stock torch optimizer keeps working on the same Parameters
    before = pol.model.action_head.weight.detach().clone()
    torch.optim.AdamW(pol.parameters(), lr=1e-2).step()
    assert not torch.equal(before, pol.model.action_head.weight.detach())
    views = pol.model._engine().head_views(pol.model._flat)
    assert views["action_head.weight"].data_ptr() == pol.model.action_head.weight.data_ptr()
    pol.zero_grad()


def test_select_action_and_eval_forward(pol):
    batch = _batch(1)
    head_p = {k: v.detach().cpu().clone() for k, v in zip(HEAD_KEYS, pol.model.head_parameters())}
    act = pol.select_action(batch["images"][0, -1], batch["states"][0, -1], "stack the red block", torch.device(DEV))
    torch.cuda.synchronize()
    assert act.shape == (14,) and not pol.training
    pooled, states = _oracle_actions(pol, {**batch, "tasks": ["stack the red block"]}, head_p)
    check_close(act.cpu()[None], head.head_forward(head_p, pooled, states), rel=5e-3, amax=2e-2, what="select_action")


def test_fused_train_step_matches_oracle_step(pol):
    batch = _batch()
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    pol.train()
    head_p = {k: v.detach().cpu().clone() for k, v in zip(HEAD_KEYS, pol.model.head_parameters())}
    pol._opt_state = None
    # the pooled feature the HIP backbone produces for this batch (checked against the oracle backbone below); feeding
    # it to the oracle head isolates the step arithmetic: Adam's first update is lr*sign(g), so bf16 noise in the
    # feature would flip signs of near-zero gradients
    tasks = pol.processor.prepare_tasks(batch["tasks"], 3)
    with torch.no_grad():
        pooled_hip = pol.model.features(pol.processor.prepare_images(dbatch["images"], torch.device(DEV)), tasks).cpu()
    out = pol.fused_train_step(dbatch, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    torch.cuda.synchronize()
    pooled, states = _oracle_actions(pol, batch, head_p)
    assert rel_l2(pooled_hip, pooled) < 5e-3
    pred, cache = head.head_forward(head_p, pooled_hip, states, keep_cache=True)
    loss, grads = head.head_mse_backward(head_p, cache, pred, batch["actions"])
    clipped, norm = head.clip_grad_norm(grads, 1.0)
    z = {k: torch.zeros_like(v) for k, v in head_p.items()}
    newp, _, _ = head.adamw_step(head_p, clipped, z, z, 1, 1e-3, (0.9, 0.95), 1e-8, 0.01)
    assert abs(float(out["loss"]) - float(loss)) <= 1e-5 * float(loss)
    assert abs(float(out["grad_norm"]) - float(norm)) <= 1e-4 * float(norm)
    for k, p in zip(HEAD_KEYS, pol.model.head_parameters()):
        upd, ref = (p.detach().cpu() - head_p[k]), (newp[k] - head_p[k])
        solid = clipped[k].abs() > 1e-7  # away from g ~ 0, where lr*g/(|g|+eps) is ill-conditioned
        assert float((upd - ref)[solid].abs().max()) <= 2e-6, k
    # second step exercises the stored moments
    out2 = pol.fused_train_step(dbatch, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    assert float(out2["loss"]) < float(out["loss"])


def test_lerobot_wrapper_forward_and_queue():
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import HAVE_LEROBOT, FeatureType, PolicyFeature
    if HAVE_LEROBOT:
        pytest.skip("covered by lerobot's own config machinery")
    feats = {"observation.images.top": PolicyFeature(FeatureType.VISUAL, (3, 64, 64)),
             "observation.state": PolicyFeature(FeatureType.STATE, (14,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=32, dropout=0.0, input_features=feats,
                   output_features={"action": PolicyFeature(FeatureType.ACTION, (14,))})
    pol = LRPolicy(cfg).to(DEV)
    g = torch.Generator().manual_seed(1)
    batch = {"observation.images.top": torch.rand(2, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(2, 14, generator=g).to(DEV),
             "action": torch.randn(2, 1, 14, generator=g).to(DEV), "task": "push"}
    loss, info = pol.forward(batch)
    loss.backward()
    assert info["loss"] == info["mse"] == pytest.approx(float(loss)) and pol.model.action_head.weight.grad is not None
    chunk = pol.predict_action_chunk(batch)
    assert chunk.shape == (2, 1, 14)
    a = pol.select_action(batch)
    assert a.shape == (2, 14) and torch.allclose(a, chunk[:, 0])


def test_prompt_feature_cache_matches_uncached():
    """SURVEY 8f rank 1 extension (off by default): cached pooled features and the skipped tower leave the actions
    bit-identical to the uncached literal path, for hits, misses and mixed batches."""
    from vla_fastvlm.model.fastvlm_adapter import FastVLMBackbone, FastVLMBackboneConfig
    torch.manual_seed(5)
    bb = FastVLMBackbone(FastVLMBackboneConfig(model_id="synthetic:tiny:3"))
    eng = bb.engine()
    B, T = 4, 12
    vocab = eng.model.llm.vocab
    ids = torch.randint(0, vocab, (B, T), device=eng.device, dtype=torch.int32)
    mask = torch.ones(B, T, dtype=torch.int32, device=eng.device)
    mask[1, 7:] = 0
    images = torch.rand(B, 3, 40, 52)
    ref = bb.forward_ids(images, ids, mask).clone()
    bb.cache_prompt_features = True
    bb.skip_unused_tower = True
    first = bb.forward_ids(images, ids, mask)           # all misses
    again = bb.forward_ids(images, ids, mask)           # all hits: no decoder launch
    ids2 = ids.clone()
    ids2[2] = torch.randint(0, vocab, (T,), device=eng.device, dtype=torch.int32)
    mixed = bb.forward_ids(images, ids2, mask)          # one miss among hits
    torch.cuda.synchronize()
    assert torch.equal(first, ref) and torch.equal(again, ref)
    assert torch.equal(mixed[[0, 1, 3]], ref[[0, 1, 3]]) and not torch.equal(mixed[2], ref[2])
    bb.cache_prompt_features = False
    bb.skip_unused_tower = False
    assert torch.equal(bb.forward_ids(images, ids2, mask), mixed)


def test_backbone_normalize_imagenet_is_plumbed():
    """SURVEY 8 a7 / VERDICT r5 #5: `normalize_imagenet=True` (reference model/fastvlm_adapter.py:463-477, applied at :487 after the letterbox) no longer raises: the
    backbone's pixels are the oracle's letterbox + normalisation (torchvision branch: what an installed reference runs), and the pooled features change with it."""
    from oracle import preprocess
    from vla_fastvlm.model.fastvlm_adapter import FastVLMBackbone, FastVLMBackboneConfig
    torch.manual_seed(9)
    bb = FastVLMBackbone(FastVLMBackboneConfig(model_id="synthetic:tiny:3", normalize_imagenet=True, pad_value=0.5))
    plain = FastVLMBackbone(FastVLMBackboneConfig(model_id="synthetic:tiny:3", pad_value=0.5))
    S = int(bb.expected_size)
    for img in (torch.rand(2, 3, 40, 52), torch.rand(2, 3, 40, 52) * 255.0, (torch.rand(2, 30, 44, 3) * 255).to(torch.uint8)):
        pix = bb._prepare_images_tensor(img, DEV)
        torch.cuda.synchronize()
        x = img.permute(0, 3, 1, 2) if img.shape[-1] == 3 else img
        ref = preprocess.prepare_images(x.float(), S, 0.5, True, normalize=True, torchvision_branch=True)
        got = pix.float().cpu()[..., :3].permute(0, 3, 1, 2)
        assert float((got - ref).abs().max()) <= 1e-2 * max(1.0, float(ref.abs().max()))
        assert not torch.equal(pix, plain._prepare_images_tensor(img, DEV))


# ------------------------------------------------------------------------------------------------ round 2: step body
def _dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _fresh(seed=31, dropout=0.0):
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=dropout)).to(DEV)


def _half(batch, lo, hi):
    return {k: (v[lo:hi] if torch.is_tensor(v) else v[lo:hi]) for k, v in batch.items()}


def test_loss_scaled_backward_matches_scaled_gradients(pol):
    """the upstream dL/dloss (e.g. a loss weight, or accelerate's 1/accumulation) reaches the head gradients: fv_grad_scale"""
    batch = _dev(_batch())
    pol.train()
    pol.zero_grad()
    pol.compute_loss(batch)["loss"].backward()
    g1 = [p.grad.detach().clone() for p in pol.model.head_parameters()]
    pol.zero_grad()
    (0.25 * pol.compute_loss(batch)["loss"]).backward()
    torch.cuda.synchronize()
    for a, p in zip(g1, pol.model.head_parameters()):
        assert torch.allclose(p.grad, 0.25 * a, rtol=1e-6, atol=1e-9)
    pol.zero_grad()
    with torch.no_grad():  # evaluation path: no graph, same number
        out = pol.compute_loss(batch)
    assert not out["loss"].requires_grad and torch.isfinite(out["loss"])


def test_gradient_accumulation_equals_full_batch():
    """reference training/trainer.py:96,171: k micro-batches accumulated (mean of the micro-batch gradients) then ONE
    clip + AdamW step == the step on the concatenated batch (equal micro-batch sizes, MSE is a mean)."""
    batch = _batch(B=4 if False else 3)
    batch = {"images": torch.cat([batch["images"], batch["images"][:1]]), "states": torch.cat([batch["states"], batch["states"][:1]]),
             "actions": torch.cat([batch["actions"], -batch["actions"][:1]]), "tasks": batch["tasks"] + ["again"]}
    kw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    a, b = _fresh(), _fresh()
    a.train(), b.train()
    full = a.fused_train_step(_dev(batch), **kw)
    o1 = b.fused_train_step(_dev(_half(batch, 0, 2)), grad_accum_steps=2, **kw)
    before = b.model._flat.clone()
    assert not o1["synced"] and torch.equal(before, b.model.materialize())  # no update on the first micro-batch
    o2 = b.fused_train_step(_dev(_half(batch, 2, 4)), grad_accum_steps=2, **kw)
    torch.cuda.synchronize()
    assert full["synced"] and o2["synced"]
    assert abs(float(full["grad_norm"]) - float(o2["grad_norm"])) <= 2e-5 * float(full["grad_norm"])
    assert float((a.model._flat - b.model._flat).abs().max()) <= 2e-6
    assert abs(0.5 * (float(o1["loss"]) + float(o2["loss"])) - float(full["loss"])) <= 1e-5 * abs(float(full["loss"]))
    # a ragged tail: force_sync applies the update with accelerate's fixed 1/k scale
    o3 = b.fused_train_step(_dev(_half(batch, 0, 2)), grad_accum_steps=2, force_sync=True, **kw)
    assert o3["synced"] and b._opt_state["step"] == 2 and b._opt_state["micro"] == 0


def test_pipelined_steps_equal_serial_steps():
    """the look-ahead loop (batch k+1's frozen forward enqueued before the optimiser waits on batch k's exchange) changes the
    order of independent work only: parameters after 3 steps are bit-identical to the serial loop."""
    batches = [_dev(_half(_batch(), i, i + 2)) for i in (0, 1)] + [_dev(_batch())]
    kw = dict(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    a, b = _fresh(41, 0.1), _fresh(41, 0.1)
    a.train(), b.train()
    for bt in batches:
        a.fused_train_step(bt, **kw)
    prepared = None
    for i, bt in enumerate(batches):
        nxt = batches[i + 1] if i + 1 < len(batches) else None
        out = b.fused_train_step(bt if prepared is None else None, prepared=prepared, next_batch=nxt, **kw)
        prepared = out["next"]
    torch.cuda.synchronize()
    assert prepared is None and torch.equal(a.model._flat, b.model._flat)


def test_trainer_resume_restores_optimizer_state(tmp_path):
    """save -> load -> one step == uninterrupted training (AdamW moments, bias-correction step and the LR index
    come back; reference trainer.py:257-262 restores them through accelerator.load_state)."""
    from vla_fastvlm.training import Trainer, TrainingConfig
    data = [_half(_batch(), 0, 2), _half(_batch(), 1, 3), _batch(), _half(_batch(), 0, 2)]
    cfg = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1000, eval_steps=1000, seed=1)
    a = _fresh(51)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=4, **cfg)).fit()
    b = _fresh(51)
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=4, **cfg))
    tb.num_training_steps = 4
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    assert (ck / "optimizer.pt").is_file() and (ck / "policy_state_dict.pt").is_file()
    c = _fresh(99)  # different init: everything must come from the checkpoint
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=4, resume_from=str(ck), **cfg))
    tc.fit()
    torch.cuda.synchronize()
    assert tc.update_step == 4 and c._opt_state["step"] == 4
    assert float((a.model._flat - c.model._flat).abs().max()) <= 1e-7


def test_last_error_is_per_handle_and_comm_world1():
    from fastvla_hip import FastVLAEngine, _lib
    m = arch.preset("tiny")
    e1 = FastVLAEngine(m, hidden_dim=32, fusion_dim=32, max_batch=2, max_text_tokens=8)
    e2 = FastVLAEngine(m, hidden_dim=32, fusion_dim=32, max_batch=2, max_text_tokens=8)
    lib = e1.lib
    assert lib.fv_workspace_bytes(e1.h, -1, 4, 0, None) != 0          # error on handle 1
    assert lib.fv_bind_workspace(e2.h, 12345, 64) != 0                # a different error on handle 2
    m1, m2 = lib.fv_last_error(e1.h).decode(), lib.fv_last_error(e2.h).decode()
    assert "fv_workspace_bytes" in m1 and "aligned" in m2 and m1 != m2
    # RCCL entry points: a one-rank communicator on this GPU, all-reduce is the identity
    uid = e1.comm_unique_id()
    comm = e1.comm_init(uid, 0, 1)
    g = torch.arange(16, dtype=torch.float32, device=DEV)
    e1.allreduce_grads(comm, g)
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), torch.arange(16, dtype=torch.float32))
    e1.comm_destroy(comm)
    e1.close(), e2.close()


def test_folded_dataset_normalisation_matches_the_processor_arithmetic():
    """STATE (x - mean) / (std + 1e-8) ahead of the policy and ACTION a * std + mean behind it -- what LeRobot's
    Normalizer / Unnormalizer steps do (reference lerobot_fastvla/processor_fastvla.py:34-48) -- folded into the head kernels:
    raw states in, un-normalised actions out, bit-for-bit the unfolded policy fed normalised states, up to the fp32 rounding of
    the affine maps; training keeps its loss in normalised space."""
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import HAVE_LEROBOT, FeatureType, PolicyFeature
    if HAVE_LEROBOT:
        pytest.skip("stand-in semantics are only exercised without lerobot")
    feats = {"observation.images.top": PolicyFeature(FeatureType.VISUAL, (3, 64, 64)), "observation.state": PolicyFeature(FeatureType.STATE, (6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats,
                   output_features={"action": PolicyFeature(FeatureType.ACTION, (5,))}, dropout=0.0)
    torch.manual_seed(3)
    pol = LRPolicy(cfg).to(DEV)
    g = torch.Generator().manual_seed(4)
    stats = {"observation.state": {"mean": torch.randn(6, generator=g), "std": torch.rand(6, generator=g) + 0.5},
             "action": {"mean": torch.randn(5, generator=g), "std": torch.rand(5, generator=g) + 0.5}}
    raw = torch.randn(3, 6, generator=g) * 2 + 1
    batch = {"observation.images.top": torch.rand(3, 3, 64, 64, generator=g).to(DEV), "task": ["a", "b", "c"]}
    norm_state = (raw - stats["observation.state"]["mean"]) / (stats["observation.state"]["std"] + 1e-8)
    pol.reset()
    a_norm = pol.select_action({**batch, "observation.state": norm_state.to(DEV)}).cpu()
    ref = a_norm * stats["action"]["std"] + stats["action"]["mean"]
    pol.fold_dataset_stats(stats)
    pol.reset()
    a_fold = pol.select_action({**batch, "observation.state": raw.to(DEV)}).cpu()
    assert float((a_fold - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    # ... and against the ORACLE head (oracle/head.py, pinned by the reference's goldens) fed the normalised states, with LeRobot's
    # un-normalisation applied in torch: the folded kernels are not only self-consistent, they compute the processors' arithmetic
    head_p = {k: v.detach().cpu().clone() for k, v in zip(HEAD_KEYS, pol.model.head_parameters())}
    with torch.no_grad():
        pooled = pol.model.features(batch["observation.images.top"], ["a\n", "b\n", "c\n"]).cpu()
    ref_oracle = head.head_forward(head_p, pooled, norm_state) * stats["action"]["std"] + stats["action"]["mean"]
    assert float((a_fold - ref_oracle).abs().max()) <= 1e-4 * float(ref_oracle.abs().max())
    # training: loss against NORMALISED targets, states raw -- equals the unfolded loss on normalised states
    tgt = torch.randn(3, 1, 5, generator=g)
    pol.train()
    loss_fold, _ = pol.forward({**batch, "observation.state": raw.to(DEV), "action": tgt.to(DEV)})
    pol.fold_dataset_stats(None)
    loss_ref, _ = pol.forward({**batch, "observation.state": norm_state.to(DEV), "action": tgt.to(DEV)})
    torch.cuda.synchronize()
    assert abs(float(loss_fold) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    loss_oracle = head.mse(head.head_forward(head_p, pooled, norm_state), tgt[:, 0])
    assert abs(float(loss_fold) - float(loss_oracle)) <= 1e-4 * abs(float(loss_oracle))
    # EVAL mode with autograd on: the library's backward differentiates the head, not the folded `* std + mean` behind it,
    # so the library returns normalised actions and the module finishes the un-normalisation in torch -- the SAME space as under
    # torch.no_grad() (select_action above), still differentiable; the statistics survive a state_dict round trip
    pol.fold_dataset_stats(stats)
    pol.eval()
    a_eval = pol._predict_actions({**batch, "observation.state": raw.to(DEV)})
    assert a_eval.requires_grad
    assert float((a_eval.detach().cpu() - ref_oracle).abs().max()) <= 1e-4 * float(ref_oracle.abs().max())
    with torch.no_grad():
        a_nograd = pol._predict_actions({**batch, "observation.state": raw.to(DEV)})
    assert float((a_eval.detach() - a_nograd).abs().max()) <= 2e-6 * float(ref_oracle.abs().max())
    a_eval.sum().backward()      # d(sum a * std + mean) reaches the head parameters
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in pol.model.head_parameters())
    pol.zero_grad(set_to_none=True)
    sd = pol.state_dict()
    assert "model.backbone.io_norm.action_std" in sd
    pol.fold_dataset_stats(None)
    pol.load_state_dict(sd)
    pol.reset()
    a_again = pol.select_action({**batch, "observation.state": raw.to(DEV)}).cpu()
    assert torch.equal(a_again, a_fold)


def test_bench_gpus2_spawns_two_ranks_and_fills_train_dp():
    """`python bench.py --gpus 2` (no torchrun) must run TWO ranks: the parent spawns them before any GPU call,
    rank 0's JSON line comes back with n_gpus = 2 and a filled train_dp (gloo here: two ranks share this box's one GPU, so RCCL
    cannot form a communicator; the exchange / overlap fields are exercised all the same)."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--backend", "gloo", "--model", "tiny", "--batch", "4",
                        "--train-batch", "4", "--tokens", "16", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 8
    assert line["dist"]["world_size"] == 2 and line["dist"]["backend"] == "gloo"
    td = line["train_dp"]
    assert td["parallelism"] == "dp2" and td["global_batch"] == 8 and td["value"] > 0
    assert td["allreduce_ms"] is not None and td["ms_per_step_serial_exchange"] is not None and td["overlap_frac"] is not None


def test_bench_gpus2_unfrozen_legs_exchange_their_buckets():
    """`bench.py --gpus 2 --train-unfrozen-dp`: both unfrozen legs (decoder + projector + head; everything incl. the FastViT-HD tower) run on TWO ranks with
    the per-bucket exchange under the backward pass (gloo: the ranks share this box's one GPU) -- the N > 1 form of SURVEY 8f-4 that the 8-GPU node will run."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--backend", "gloo", "--model", "small", "--batch", "4", "--train-batch", "4",
                        "--unfrozen-batch", "2", "--tokens", "16", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-surface", "--train-unfrozen-dp", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2
    for leg in ("train_unfrozen", "train_unfrozen_tower"):
        t = line[leg]
        assert t is not None and "error" not in t, t
        assert t["parallelism"] == "dp2" and t["global_batch"] == 4 and t["value"] > 0 and t["collectives_per_step"] >= 2
        # what the per-bucket exchange still exposes = the step with its collectives minus the same step without them
        assert isinstance(t["exchange"]["exchange_exposed_ms"], float) and t["exchange"]["ms_per_step_without_exchange"] > 0
    d = line["dist"]
    assert d["world_size"] == 2 and d["deadline_hit"] is False and d["fv_comm"]["ok"] is None and "RCCL" in d["fv_comm"]["skipped"]   # gloo rehearsal: no RCCL communicator
    assert line["train_dp"]["allreduce_ms"] is not None and line["train_dp"]["overlap_frac"] is not None
    assert line["train_unfrozen_tower"]["buckets"] > line["train_unfrozen"]["buckets"] and line["train_unfrozen_tower"]["fp16_saturations"] == 0


def test_bench_gpus2_deadline_prints_the_headline_and_leaves():
    """the legs behind the headline measurement of an N > 1 run sit under a watchdog (`--secondary-deadline`): past it rank 0 prints the line with what it
    has (`dist.deadline_hit`), every rank leaves by itself, the launcher sees exit code 0 -- a stalled secondary leg can delay a scaling run, never lose it."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--backend", "gloo", "--model", "tiny", "--batch", "4", "--train-batch", "4",
                        "--tokens", "16", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--secondary-deadline", "0.02", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["roofline"] is not None
    assert line["dist"]["deadline_hit"] is True and line["dist"]["world_size"] == 2


def test_bench_plain_run_times_the_steps_and_dumps_the_actions(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: the headline fields only (every secondary leg null), the timed step
    count as asked, and the last timed step's actions as DIR/actions.npy (float32, (batch, 14))."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    import numpy as np
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--model", "tiny", "--batch", "4", "--tokens", "16", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["ms_per_step"] - 1e3 / line["value"]) <= 1e-2 * line["ms_per_step"] + 1e-3
    assert line["unit"] == "steps/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    for leg in ("roofline", "power", "cpu_baseline", "cpu_baseline_c1", "train_dp", "train_unfrozen", "train_unfrozen_tower", "surface",
                "other_parity_mode", "families", "gemm_shapes"):
        assert line[leg] is None, leg
    a = np.load(out / "actions.npy")
    assert a.dtype == np.float32 and a.shape == (4, 14) and np.isfinite(a).all() and np.abs(a).max() > 0


def test_image_prefix_cache_in_the_backbone():
    """SURVEY.md 8f-1 through the plugin-side class: FastVLMBackbone in splice mode with `cache_image_prefix` keeps every image's
    decoder prefix (LRU keyed by a device-side hash of the image tensor).  Misses, hits, a frame repeated inside one batch and a
    mixed batch all give the pooled rows of the uncached spliced forward; on hits neither the tower nor the prefix pass runs."""
    from vla_fastvlm.model.fastvlm_adapter import FastVLMBackbone, FastVLMBackboneConfig
    torch.manual_seed(8)
    bb = FastVLMBackbone(FastVLMBackboneConfig(model_id="synthetic:small:5"))
    bb.splice_image_tokens = True
    eng = bb.engine()
    B, T = 4, 12
    vocab = eng.model.llm.vocab
    ids = torch.randint(0, vocab, (B, T), device=eng.device, dtype=torch.int32)
    mask = torch.ones(B, T, dtype=torch.int32, device=eng.device)
    mask[2, 5:] = 0
    images = torch.rand(B, 3, 60, 84, device=eng.device)
    images[3] = images[1]                                   # the same frame twice in one batch
    ref = bb.forward_ids(images, ids, mask).clone()
    calls = {"n": 0, "imgs": 0}
    vf = eng.vision_forward

    def counted(pix, *a, **k):
        calls["n"] += 1
        calls["imgs"] += pix.shape[0]
        return vf(pix, *a, **k)

    eng.vision_forward = counted
    bb.cache_image_prefix = True
    first = bb.forward_ids(images, ids, mask)               # 3 distinct frames miss
    assert calls == {"n": 1, "imgs": 3} and bb._prefix_stats == {"images": 4, "tower_runs": 3}
    again = bb.forward_ids(images, ids, mask)               # all hits: no tower, no prefix pass
    assert calls == {"n": 1, "imgs": 3} and bb._prefix_stats["tower_runs"] == 0
    ids2 = torch.randint(0, vocab, (B, T), device=eng.device, dtype=torch.int32)
    other = bb.forward_ids(images, ids2, mask)              # new prompts on cached frames
    images2 = images.clone()
    images2[0] = torch.rand(3, 60, 84, device=eng.device)
    mixed = bb.forward_ids(images2, ids, mask)              # one new frame among hits
    torch.cuda.synchronize()
    assert calls == {"n": 2, "imgs": 4}
    bb.cache_image_prefix = False
    eng.vision_forward = vf
    tol = 1e-3 if eng.llm_precision == 2 else 2e-5
    assert rel_l2(first.cpu(), ref.cpu()) <= tol and torch.equal(first, again)
    assert rel_l2(other.cpu(), bb.forward_ids(images, ids2, mask).cpu()) <= tol
    assert rel_l2(mixed.cpu(), bb.forward_ids(images2, ids, mask).cpu()) <= tol
    assert torch.equal(mixed[1:], first[1:]) and not torch.equal(mixed[0], first[0])
