"""-m gpu: action chunks -- the chunked loss kernel against float64, the bit rules of the default path, the head step against autograd, the denominator under
gradient accumulation, backbone training (full, LoRA projected, LoRA direct), the policy surfaces and checkpoints.

Bars (the project's own): loss and metrics relative 1e-5 (the fixed-order fp32 norms, the head-golden loss); dL/dactions per element
|d| <= 2e-5 max(1e-3 max|ref|, |ref|); head gradients 2e-5 max(1e-3, max|ref|) per tensor (the head goldens); backbone gradients rel_l2 2e-3."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from chunk_loss_util import KINDS, chunk_loss_ref, ragged_pad, torch_loss_ref  # noqa: E402
from gpu_util import DEV, call, lib, rel_l2, stream  # noqa: E402
from fastvla_hip import HEAD_KEYS, FastVLAEngine, _lib, arch, lora, weights  # noqa: E402
from oracle import head, qwen2, train_unfrozen  # noqa: E402
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy  # noqa: E402

KIND_ID = _lib.LOSS_KINDS
BETA = 0.5


# ------------------------------------------------------------------------------------------------------------------ 1. the loss kernel against float64
def _op_loss(a, t, pad, kind, beta=BETA, loss_scale=1.0):
    """chunk_loss_kernel + fold alone (fv_op_chunk_loss): a, t (B, K, A) f32 CPU, pad (B, K) bool or None -> loss, metrics (2,), g (B, K, A) on the CPU"""
    B, K, A = a.shape
    ad, td = a.to(DEV).contiguous(), t.to(DEV).contiguous()
    pd = None if pad is None else torch.as_tensor(pad).to(DEV, torch.uint8).contiguous()
    g = torch.full((B, K, A), float("nan"), device=DEV)
    part, out = torch.full((768,), float("nan"), device=DEV), torch.full((3,), float("nan"), device=DEV)
    call(lib().fv_op_chunk_loss(ad.data_ptr(), td.data_ptr(), None if pd is None else pd.data_ptr(), g.data_ptr(), part.data_ptr(), part.numel(), out.data_ptr(),
                                out[1:].data_ptr(), a.numel(), A, KIND_ID[kind], beta, loss_scale, stream()), "fv_op_chunk_loss")
    torch.cuda.synchronize()
    return float(out[0]), out[1:].cpu(), g.cpu()


def _loss_inputs(B, K, A, seed):
    """random actions / targets in fp32 whose differences are exact in fp32 where it matters: d == 0, |d| == beta, and |d| one ulp on either side of beta"""
    g = torch.Generator().manual_seed(seed)
    a, t = torch.randn(B, K, A, generator=g), torch.randn(B, K, A, generator=g)
    n = a.numel()
    if n >= 8:
        af, tf = a.view(-1), t.view(-1)
        lo, hi = float(np.nextafter(np.float32(BETA), np.float32(0))), float(np.nextafter(np.float32(BETA), np.float32(1)))
        for i, d in enumerate((0.0, BETA, -BETA, lo, -lo, hi, -hi)):
            j = (i * 5) % n if n >= 35 else i
            af[j] = 0.5
            tf[j] = 0.5 - d          # 0.5 - (0.5 - d) == d exactly for these d
    return a, t


def _masks(B, K, t):
    """name -> (pad, targets): all valid, a ragged trailing pad per row, all padded, and the ragged pad with NaN / +inf / -inf written into the padded targets"""
    rag = ragged_pad(B, K, seed=1) if B * K > 1 else np.ones((B, K), dtype=bool)
    poisoned = t.clone()
    vals = torch.tensor([float("nan"), float("inf"), float("-inf")])
    sel = torch.from_numpy(rag).unsqueeze(-1).expand_as(t)
    poisoned[sel] = vals[torch.arange(int(sel.sum())) % 3]
    return {"none": (None, t), "all-valid": (np.zeros((B, K), dtype=bool), t), "ragged": (rag, t), "all-padded": (np.ones((B, K), dtype=bool), t),
            "ragged-nan-inf": (rag, poisoned)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 5), (2, 7, 3), (9, 7, 14), (64, 50, 14)])
def test_loss_kernel_matches_float64(shape, kind):
    B, K, A = shape
    a, t0 = _loss_inputs(B, K, A, seed=B * 100 + K)
    n = a.numel()
    worst = {"loss": 0.0, "mse": 0.0, "g": 0.0}
    for ls in (1.0, 4096.0):
        for name, (pad, t) in _masks(B, K, t0).items():
            loss, met, g = _op_loss(a, t, pad, kind, loss_scale=ls)
            ref = chunk_loss_ref(a.numpy(), t.numpy(), pad, kind, BETA, loss_scale=ls)
            assert np.isfinite(loss) and torch.isfinite(met).all() and torch.isfinite(g).all(), (name, "non-finite")
            for what, got, want in (("loss", loss, ref["loss"]), ("mse", float(met[0]), ref["mse"]), ("valid", float(met[1]), ref["valid"])):
                err = abs(got - want) / abs(want) if want else abs(got)
                if what in worst:
                    worst[what] = max(worst[what], err / 1e-5)
                assert err <= 1e-5, (name, what, got, want)
            rg = torch.from_numpy(ref["g"])
            bar = 2e-5 * torch.maximum(1e-3 * rg.abs().max(), rg.abs())
            diff = (g.double() - rg).abs()
            if float(rg.abs().max()) > 0:
                worst["g"] = max(worst["g"], float((diff / bar).max()))
            assert bool((diff <= bar).all()), (name, "g", float((diff / bar.clamp_min(1e-300)).max()))
            if pad is not None:
                assert bool((g[torch.from_numpy(pad)] == 0).all()), name           # a padded step gets exactly 0, whatever its target holds
            if name == "all-padded":
                assert loss == 0.0 and float(met[0]) == 0.0 and float(met[1]) == 0.0 and bool((g == 0).all())
            if kind == "l1":       # sign(d) / n: the three values loss_scale / n (one fp32 division), its negative and 0 -- exactly
                c = float(np.float32(ls) / np.float32(n))
                d = (a.double() - torch.nan_to_num(t.double(), nan=0.0, posinf=0.0, neginf=0.0))
                want = torch.zeros_like(d)
                want[d > 0], want[d < 0] = c, -c
                if pad is not None:
                    want = torch.where(torch.from_numpy(pad).unsqueeze(-1).expand_as(want), torch.zeros_like(want), want)
                assert torch.equal(g.double(), want), name
    # two runs agree bit for bit (fixed-order partials, no atomics)
    pad, t = _masks(B, K, t0)["ragged"]
    r1, r2 = _op_loss(a, t, pad, kind), _op_loss(a, t, pad, kind)
    assert r1[0] == r2[0] and torch.equal(r1[1], r2[1]) and torch.equal(r1[2], r2[2])
    print(f"[chunk loss {kind} {shape}] worst error / bar: loss {worst['loss']:.3f} masked mse {worst['mse']:.3f} g {worst['g']:.3f}")


def test_loss_kernel_unaligned_pointers_take_the_scalar_form():
    """a, t or g off a 16-byte boundary: the float4 body is not used; the result is the float64 one all the same"""
    B, K, A = 5, 3, 7
    a, t = _loss_inputs(B, K, A, seed=11)
    pad = ragged_pad(B, K, seed=2)
    n = a.numel()
    buf = torch.zeros(3, n + 4, device=DEV)
    av, tv, gv = buf[0, 1:n + 1], buf[1, 1:n + 1], buf[2, 1:n + 1]
    av.copy_(a.view(-1)), tv.copy_(t.view(-1))
    assert av.data_ptr() % 16 == 4
    pd = torch.from_numpy(pad).to(DEV, torch.uint8).contiguous()
    part, out = torch.zeros(768, device=DEV), torch.zeros(3, device=DEV)
    call(lib().fv_op_chunk_loss(av.data_ptr(), tv.data_ptr(), pd.data_ptr(), gv.data_ptr(), part.data_ptr(), 768, out.data_ptr(), out[1:].data_ptr(), n, A,
                                KIND_ID["smooth_l1"], BETA, 1.0, stream()), "fv_op_chunk_loss")
    torch.cuda.synchronize()
    ref = chunk_loss_ref(a.numpy(), t.numpy(), pad, "smooth_l1", BETA)
    assert abs(float(out[0]) - ref["loss"]) <= 1e-5 * ref["loss"]
    rg = torch.from_numpy(ref["g"]).view(-1)
    assert bool(((gv.cpu().double() - rg).abs() <= 2e-5 * torch.maximum(1e-3 * rg.abs().max(), rg.abs())).all())
    assert float(buf[2, 0]) == 0.0 and float(buf[2, n + 1]) == 0.0           # nothing written outside g


# ------------------------------------------------------------------------------------------------------------------ head rigs
FEAT, HID, FUS, DS = 48, 24, 40, 6


def _head_engine(da, B):
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=FEAT, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    return FastVLAEngine(m, state_dim=DS, action_dim=da, hidden_dim=HID, fusion_dim=FUS, max_batch=max(B, 1))


def _head_params(da, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = head.head_shapes(FEAT, DS, da, HID, FUS)
    return {k: torch.randn(*s, generator=g) * (0.2 if len(s) > 1 else 0.1) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
            for k, s in shapes.items()}


def _flat(eng, p):
    flat = torch.zeros(eng.head_numel(), device=DEV)
    for k, v in eng.head_views(flat).items():
        v.copy_(p[k])
    return flat


def _head_io(B, da, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, FEAT, generator=g), torch.randn(B, DS, generator=g), torch.randn(B, da, generator=g)


# ------------------------------------------------------------------------------------------------------------------ 2. bit rules
@pytest.mark.parametrize("K", [1, 4])
def test_default_path_keeps_its_bits_after_the_setters(K):
    A, B = 5, 3
    da = K * A
    p = _head_params(da, 3)
    pooled, states, tgt = _head_io(B, da, 4)
    fresh, seen = _head_engine(da, B), _head_engine(da, B)

    def step(eng, pad=None):
        flat = _flat(eng, p)
        act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
        loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved, pad=pad)
        torch.cuda.synchronize()
        return loss.clone(), grads.clone()

    l0, g0 = step(fresh)
    seen.set_head_loss("l1", 1.0, K)
    l1a, g1a = step(seen, pad=ragged_pad(B, K, seed=1))
    l1b, g1b = step(seen, pad=ragged_pad(B, K, seed=1))
    assert torch.equal(l1a, l1b) and torch.equal(g1a, g1b)                   # two calls of the new kernel
    assert not torch.equal(g1a, g0)
    seen.set_head_loss()                                                     # fv_head_set_loss(NULL); the mask was cleared after each call
    l2, g2 = step(seen)
    assert torch.equal(l2, l0) and torch.equal(g2, g0)
    # MSE through the chunked kernel (an all-valid mask) against the single-block kernel: the same numbers up to the summation order of the loss
    seen.set_head_loss("mse", 1.0, K)
    l3, g3 = step(seen, pad=np.zeros((B, K), dtype=bool))
    met = seen.head_loss_metrics().cpu()
    assert abs(float(l3) - float(l0)) <= 1e-5 * float(l0) and abs(float(met[0]) - float(l0)) <= 1e-5 * float(l0) and float(met[1]) == 1.0
    for k, v in fresh.head_views(g0).items():
        assert float((seen.head_views(g3)[k] - v).abs().max()) <= 2e-5 * max(1e-3, float(v.abs().max())), k
    print(f"[chunk bits K={K}] masked-MSE gradients equal the single-block kernel's bit for bit: {torch.equal(g3, g0)}; loss {float(l3)!r} vs {float(l0)!r}")
    fresh.close(), seen.close()


def test_setter_argument_checks_enqueue_nothing():
    eng = _head_engine(20, 2)
    L = eng.lib
    for spec in (_lib.HeadLossSpec(3, 1.0, 1), _lib.HeadLossSpec(-1, 1.0, 1), _lib.HeadLossSpec(2, 0.0, 1), _lib.HeadLossSpec(2, float("nan"), 1),
                 _lib.HeadLossSpec(0, 1.0, 0), _lib.HeadLossSpec(1, 1.0, 3), _lib.HeadLossSpec(1, 1.0, 40)):
        assert L.fv_head_set_loss(eng.h, spec) == -1, (spec.kind, spec.beta, spec.chunk)
    assert L.fv_head_set_loss(None, None) == -1 and L.fv_head_set_loss_mask(None, None) == -1 and L.fv_head_loss_metrics(eng.h, None) == -1
    assert "chunk" in L.fv_last_error(eng.h).decode() or "null" in L.fv_last_error(eng.h).decode()
    assert eng.head_loss == dict(kind="mse", beta=1.0, chunk=1)
    with pytest.raises(ValueError):
        eng.set_head_loss("l1", 1.0, 3)                                      # 20 % 3
    eng.set_head_loss("l1", 1.0, 4)
    with pytest.raises(ValueError, match="action_is_pad"):
        eng._pad_arg(np.zeros((2, 5), dtype=bool), 2)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the head step against autograd
@pytest.mark.parametrize("kind", KINDS)
def test_head_step_matches_float64_autograd(kind):
    B, K, A = 3, 4, 5
    da = K * A
    p = _head_params(da, 7)
    pooled, states, tgt = _head_io(B, da, 8)
    pad = ragged_pad(B, K, seed=1)
    eng = _head_engine(da, B)
    eng.set_head_loss(kind, BETA, K)
    flat = _flat(eng, p)
    act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
    loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved, pad=pad)
    met = eng.head_loss_metrics().cpu()
    torch.cuda.synchronize()
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    pred = head.head_forward(p64, pooled.double(), states.double())          # the unchanged oracle head, K * A wide
    ref = torch_loss_ref(pred.view(B, K, A), tgt.double().view(B, K, A), torch.from_numpy(pad), kind, BETA)
    ref.backward()
    np.testing.assert_allclose(act.cpu().numpy(), pred.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    mse = torch_loss_ref(pred.detach().view(B, K, A), tgt.double().view(B, K, A), torch.from_numpy(pad), "mse")
    assert abs(float(met[0]) - float(mse)) <= 1e-5 * float(mse) and abs(float(met[1]) - float((~pad).mean())) <= 1e-6
    gv = eng.head_views(grads)
    worst = 0.0
    for k in HEAD_KEYS:
        r = p64[k].grad
        bar = 2e-5 * max(1e-3, float(r.abs().max()))
        err = float((gv[k].cpu().double() - r).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (k, err, bar)
    print(f"[chunk head step {kind}] worst gradient error / bar {worst:.3f}")
    # all padded: loss 0.0 and every one of the 12 gradients exactly zero
    loss0, g0 = eng.head_backward(flat, act, tgt.to(DEV), saved, pad=np.ones((B, K), dtype=bool))
    torch.cuda.synchronize()
    assert float(loss0) == 0.0 and all(bool((v == 0).all()) for v in eng.head_views(g0).values())
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4. accumulation keeps the denominator
def _policy(K=4, loss="l1", n_steps=1, seed=31, model="tiny:77", hd=(48, 64), **cfg):
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{model}", hidden_dim=hd[0], fusion_dim=hd[1], dropout=0.0, **cfg), chunk_size=K,
                         n_action_steps=n_steps, action_loss=loss, action_loss_beta=BETA).to(DEV)


def _chunk_batch(B, K, A=14, seed=5, pads=None):
    g = torch.Generator().manual_seed(seed)
    pad = torch.zeros(B, K, dtype=torch.bool)
    for b, k in enumerate(pads if pads is not None else [(b + 1) % (K + 1) for b in range(B)]):
        if k:
            pad[b, K - k:] = True
    return {"images": torch.rand(B, 3, 72, 96, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, K, A, generator=g),
            "action_is_pad": pad, "tasks": ["stack the red block", "open drawer", "x", "push"][:B]}


def _dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_accumulation_keeps_the_all_element_denominator(kind):
    """rows with 0 / 1 / 3 / 4 padded steps of 4: one batch of four against the same rows as two micro-batches of two (7 valid steps, then 1).  With the
    loss divided by ALL elements the two micro-batch gradients average to the full-batch gradient; a valid-count denominator would weigh the second
    micro-batch's single valid step seven times too heavily."""
    K = 4
    batch = _dev(_chunk_batch(4, K, pads=[0, 1, 3, 4]))
    kw = dict(lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    a, b = _policy(K, kind), _policy(K, kind)
    a.train(), b.train()
    prep = a.prepare_batch(batch)          # ONE frozen forward: both policies step on the same pooled features
    assert prep["targets"].shape == (4, K * 14) and prep["pad"].shape == (4, K)
    full = a.fused_train_step(prepared=prep, **kw)
    half = [{k: v[lo:lo + 2].contiguous() for k, v in prep.items()} for lo in (0, 2)]
    o1 = b.fused_train_step(prepared=half[0], grad_accum_steps=2, **kw)
    assert not o1["synced"]
    o2 = b.fused_train_step(prepared=half[1], grad_accum_steps=2, **kw)
    torch.cuda.synchronize()
    assert full["synced"] and o2["synced"] and full["actions"].shape == (4, K, 14)
    ref, acc = a._opt_state["g"], 0.5 * b._opt_state["acc"]
    err = float((acc - ref).abs().max())
    print(f"[chunk accumulation {kind}] accumulated gradient max error {err:.3e} (bar {2e-5 * float(ref.abs().max()):.3e}); parameters max diff "
          f"{float((a.model._flat - b.model._flat).abs().max()):.3e}")
    assert err <= 2e-5 * float(ref.abs().max())
    assert float((a.model._flat - b.model._flat).abs().max()) <= 3e-7
    assert abs(0.5 * (float(o1["loss"]) + float(o2["loss"])) - float(full["loss"])) <= 1e-5 * float(full["loss"])
    # the float64 loss of the same numbers, and the masked MSE beside it
    r = chunk_loss_ref(full["actions"].cpu().numpy(), batch["actions"].cpu().numpy(), batch["action_is_pad"].cpu().numpy(), kind, BETA)
    assert abs(float(full["loss"]) - r["loss"]) <= 1e-5 * r["loss"] and abs(float(full["mse"]) - r["mse"]) <= 1e-5 * r["mse"]
    for p_ in (a, b):
        p_.model.backbone.engine().close()


# ------------------------------------------------------------------------------------------------------------------ 5. backbone training
def _train_rig(model, seed, hd, B, T, da):
    """test_gpu_train_unfrozen._rig with a head that is `da` wide"""
    w = weights.init_backbone(model, seed=seed)
    eng = FastVLAEngine(model, state_dim=14, action_dim=da, hidden_dim=hd, fusion_dim=hd, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng.load_weights(w)
    eng.train_begin()
    tensors, total, nb = eng.train_layout()
    flat = torch.zeros(total, dtype=torch.float32, device=DEV)
    eng.train_export_params(flat)
    lc = qwen2.Qwen2Cfg(hidden=model.llm.hidden, layers=model.llm.layers, heads=model.llm.heads, kv_heads=model.llm.kv_heads, head_dim=model.llm.head_dim,
                        inter=model.llm.inter, vocab=model.llm.vocab, rope_theta=model.llm.rope_theta, rms_eps=model.llm.rms_eps)
    g = torch.Generator().manual_seed(seed + 1)
    hp = {k: (torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
          for k, s in head.head_shapes(lc.hidden, 14, da, hd, hd).items()}
    for k, v in eng.head_views(flat).items():
        v.copy_(hp[k])
    return w, eng, flat, lc, hp


def test_backbone_training_with_chunks_matches_autograd(monkeypatch):
    """synthetic:small, K = 4, L1, a ragged mask: one full fine-tuning step and one rank-16 projected LoRA step against autograd (the oracles of
    test_gpu_train_unfrozen / test_gpu_lora with their one `F.mse_loss(pred, targets)` swapped for the masked L1), then the direct LoRA step against the
    projected one.  L1's derivative jumps at d = 0 and the bf16 backbone moves a prediction by ~1e-3 of its size, so the targets are placed at least 0.1
    away from the device's own predictions: no element's sign depends on the arithmetic."""
    from test_gpu_lora import _lora_oracle, _random_adapters, _trainable_named
    from test_gpu_train_unfrozen import GRAD_TOL, _check_grads, _inputs
    model = arch.preset("small")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, T, K, A, hd, rank = 3, 16, 4, 5, 64, 16
    da = K * A
    w, eng, flat, lc, hp = _train_rig(model, 41, hd, B, T, da)
    tower_out, ids, mask, states, _ = _inputs(model, B, T, 42)
    pad = ragged_pad(B, K, seed=1)
    padt = torch.from_numpy(pad)
    eng.set_head_loss("l1", 1.0, K)
    ws = eng.train_workspace(B, T)
    fg = torch.zeros_like(flat)
    act0, _, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, torch.zeros(B, da), ws, training=False, flat_grads=fg, pad=pad)
    g = torch.Generator().manual_seed(43)
    delta = (0.1 + 1.4 * torch.rand(B, da, generator=g)) * (torch.randint(0, 2, (B, da), generator=g) * 2 - 1)
    targets = act0.cpu() + delta
    monkeypatch.setattr(F, "mse_loss", lambda pred, tgt: torch_loss_ref(pred.view(B, K, A), tgt.view(B, K, A), padt, "l1"))

    # full fine-tuning
    act, loss, grads = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=fg, pad=pad)
    torch.cuda.synchronize()
    ref = train_unfrozen.forward_backward(w, hp, tower_out.float(), ids, mask, states, targets, lc)
    ra, rl = rel_l2(act.cpu(), ref["pred"]), abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    worst = _check_grads(eng, grads, ref, tol=GRAD_TOL)
    print(f"[chunk unfrozen small K={K} l1] actions rel_l2={ra:.2e} loss rel={rl:.2e} worst gradient: {worst[0]} {worst[1]:.2e}")
    assert ra <= 1e-3 and rl <= 1e-3
    assert bool((ref["pred"].view(B, K, A) - targets.view(B, K, A)).abs()[~padt].min() > 0.05)       # the construction held on the oracle's side too

    # rank-16 LoRA, projected backward
    alpha = 2.0 * rank
    eng.train_lora_begin(rank, alpha, None)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    eng.train_lora_commit(flat, lflat)
    lg = torch.zeros(ltotal, device=DEV)
    act0, _, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, torch.zeros(B, da), ws, training=False, flat_grads=fg, pad=pad)
    targets = act0.cpu() + delta
    actp, lossp, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=fg, pad=pad)
    eng.train_lora_project(fg, lflat, lg)
    torch.cuda.synchronize()
    par = {k: v.clone() for k, v in lora.adapter_views(lflat, lt).items()}
    ref = _lora_oracle(w, hp, par, alpha / rank, tower_out, ids, mask, states, targets, lc, rounded=True)
    ra, rl = rel_l2(actp.cpu(), ref["pred"]), abs(float(lossp) - float(ref["loss"])) / float(ref["loss"])
    got = _trainable_named(lg / eng.train_loss_scale(), lt)
    assert set(got) == set(ref["grads"])
    errs = sorted(((rel_l2(v.cpu(), ref["grads"][k]), k) for k, v in got.items() if float(ref["grads"][k].norm()) > 1e-12), reverse=True)
    print(f"[chunk lora small K={K} l1 r={rank}] actions rel_l2={ra:.2e} loss rel={rl:.2e}; worst gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
    assert ra <= 1e-3 and rl <= 1e-3
    for e, k in errs:
        assert e <= GRAD_TOL, f"gradient of {k}: rel_l2 {e:.3e} > {GRAD_TOL}"

    # the direct LoRA backward runs the same forward, the same loss kernel and the same head backward on the same operands: actions, loss and the head's 12
    # gradients equal the projected step's bit for bit (test_gpu_lora_direct.py's projected-vs-direct bar); a mask or spec that did not reach the direct
    # entry point would show here
    lgd = torch.full((ltotal,), float("nan"), device=DEV)
    actd, lossd, _ = eng.train_lora_forward_backward(flat, lflat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, lora_grads=lgd, pad=pad)
    torch.cuda.synchronize()
    assert torch.equal(actd, actp) and torch.equal(lossd, lossp)
    hv, hvp = eng.head_views(lgd[: eng.head_numel()]), eng.head_views(fg[: eng.head_numel()])
    assert all(torch.equal(hv[k], hvp[k]) for k in hv)
    gd = _trainable_named(lgd / eng.train_loss_scale(), lt)
    for k in ("head.action_head.weight", "head.action_head.bias"):
        assert rel_l2(gd[k].cpu(), ref["grads"][k]) <= GRAD_TOL, k
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. surfaces
def test_lerobot_surface_with_chunks():
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature      # (LeRobot's own classes where it is installed, the stand-ins otherwise)
    K, A, B = 4, 5, 2
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=3,
                   output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
    torch.manual_seed(3)
    pol = LRPolicy(cfg).to(DEV)
    g = torch.Generator().manual_seed(4)
    stats = {"observation.state": {"mean": torch.randn(6, generator=g), "std": torch.rand(6, generator=g) + 0.5},
             ACTION: {"mean": torch.randn(A, generator=g), "std": torch.rand(A, generator=g) + 0.5}}
    raw = torch.randn(B, 6, generator=g) * 2 + 1
    batch = {"observation.images.top": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "observation.state": raw.to(DEV), "task": ["a", "b"]}
    pol.fold_dataset_stats(stats)
    chunk = pol.predict_action_chunk(batch)
    assert chunk.shape == (B, K, A)
    head_p = {k: v.detach().cpu().double() for k, v in zip(HEAD_KEYS, pol.model.head_parameters())}
    with torch.no_grad():
        pooled = pol.model.features(batch["observation.images.top"], ["a\n", "b\n"]).cpu().double()
    norm_state = (raw.double() - stats["observation.state"]["mean"].double()) / (stats["observation.state"]["std"].double() + 1e-8)
    ref = head.head_forward(head_p, pooled, norm_state).view(B, K, A) * stats[ACTION]["std"].double() + stats[ACTION]["mean"].double()   # std[a], mean[a] per action dimension
    np.testing.assert_allclose(chunk.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5)
    # 7 select_action calls at n_action_steps = 3: the backbone (and the head) run 3 times, and rows 0, 1, 2 of each chunk are served in order
    eng = pol.model.backbone.engine()
    counts = {"features": 0, "head": 0}
    feats_fn, head_fn = pol.model.features, eng.head_forward
    pol.model.features = lambda *a, **k: (counts.__setitem__("features", counts["features"] + 1), feats_fn(*a, **k))[1]
    eng.head_forward = lambda *a, **k: (counts.__setitem__("head", counts["head"] + 1), head_fn(*a, **k))[1]
    pol.reset()
    got = [pol.select_action(batch) for _ in range(7)]
    assert counts == {"features": 3, "head": 3}
    for i, a_ in enumerate(got):
        assert a_.shape == (B, A) and torch.equal(a_, chunk[:, i % 3]), i      # (the same observation every time: every chunk is the one above)
    pol.model.features, eng.head_forward = feats_fn, head_fn
    # forward(batch) with action_is_pad: the loss of the float64 definition on the same numbers (normalised space: targets arrive normalised)
    tgt = torch.randn(B, K, A, generator=g)
    pad = torch.from_numpy(ragged_pad(B, K, seed=2))
    pol.set_action_loss("smooth_l1", BETA)
    pol.train()
    loss, info = pol.forward({**batch, ACTION: tgt.to(DEV), "action_is_pad": pad.to(DEV)})
    loss.backward()
    with torch.no_grad():      # the normalised predictions that loss was taken of (the same kernels on the same inputs)
        loss2, pred = pol.model.forward_loss(batch["observation.images.top"], batch["observation.state"], ["a\n", "b\n"], tgt.to(DEV), pad=pad.to(DEV))
    torch.cuda.synchronize()
    assert pred.shape == (B, K, A) and torch.equal(loss2, loss.detach())
    np.testing.assert_allclose(pred.cpu().numpy(), head.head_forward(head_p, pooled, norm_state).view(B, K, A).numpy(), rtol=1e-4, atol=1e-5)
    r = chunk_loss_ref(pred.cpu().numpy(), tgt.numpy(), pad.numpy(), "smooth_l1", BETA)
    assert abs(float(loss.detach()) - r["loss"]) <= 1e-5 * r["loss"] and info["loss"] == pytest.approx(float(loss.detach()))
    assert abs(info["mse"] - r["mse"]) <= 1e-5 * r["mse"] and info["mse"] != info["loss"]
    assert pol.model.action_head.weight.grad is not None and pol.model.action_head.weight.grad.shape == (K * A, 48)
    with pytest.raises(ValueError):
        pol.forward({**batch, ACTION: tgt[:, 0].to(DEV)})                   # (B, A) targets with K > 1
    eng.close()
    # chunk_size = 1: the (B, 1) action_is_pad every LeRobot dataset delivers is not passed on -- the plain MSE kernel, loss == mse, the mask-free run's bits
    torch.manual_seed(3)
    one = LRPolicy(LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, dropout=0.0,
                            output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))})).to(DEV)
    one.train()
    l_mask, info = one.forward({**batch, ACTION: tgt[:, :1].to(DEV), "action_is_pad": torch.zeros(B, 1, dtype=torch.bool, device=DEV)})
    l_none, _ = one.forward({**batch, ACTION: tgt[:, :1].to(DEV)})
    assert one.model.last_loss_metrics is None and info["loss"] == info["mse"] and torch.equal(l_mask.detach(), l_none.detach())
    one.model.backbone.engine().close()


def test_core_select_action_chunk_and_queue():
    pol = _policy(4, "mse", n_steps=2)
    g = torch.Generator().manual_seed(9)
    img, st = torch.rand(3, 72, 96, generator=g), torch.randn(14, generator=g)
    chunk = pol.select_action_chunk(img, st, "stack the red block", torch.device(DEV))
    assert chunk.shape == (4, 14) and not pol.training
    pol.reset()
    a0, a1 = pol.select_action(img, st, "stack the red block", torch.device(DEV)), pol.select_action(img, st, "stack the red block", torch.device(DEV))
    assert torch.equal(a0, chunk[0]) and torch.equal(a1, chunk[1]) and len(pol._action_queue) == 0
    batch = _dev(_chunk_batch(3, 4))
    assert pol.forward(batch["images"], batch["states"], batch["tasks"]).shape == (3, 4, 14)
    out = pol.compute_loss(batch)
    r = chunk_loss_ref(pol.forward(batch["images"], batch["states"], batch["tasks"]).detach().cpu().numpy(), batch["actions"].cpu().numpy(),
                       batch["action_is_pad"].cpu().numpy(), "mse")
    assert abs(float(out["loss"].detach()) - r["loss"]) <= 1e-5 * r["loss"] and abs(float(out["mse"]) - r["mse"]) <= 1e-5 * r["mse"]
    pol.model.backbone.engine().close()


# ------------------------------------------------------------------------------------------------------------------ 7. checkpoints
def test_checkpoint_round_trip_and_trainer_resume(tmp_path):
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils import load_policy_from_checkpoint
    from vla_fastvlm.utils.checkpoint import save_policy_checkpoint
    K = 4
    pol = _policy(K, "l1", n_steps=3, seed=51)
    g = torch.Generator().manual_seed(9)
    img, st = torch.rand(3, 72, 96, generator=g), torch.randn(14, generator=g)
    chunk = pol.select_action_chunk(img, st, "open drawer", torch.device(DEV))
    d = save_policy_checkpoint(pol, tmp_path / "ck")
    assert json.loads((d / "hip_extras.json").read_text()) == {"splice_image_tokens": False, "train_backbone": False, "train_tower": False,
                                                                "action_chunk": {"chunk_size": K, "n_action_steps": 3, "loss": "l1", "beta": BETA}}
    again = load_policy_from_checkpoint(str(d)).to(DEV)
    assert (again.chunk_size, again.n_action_steps, again.model.action_loss) == (K, 3, "l1")
    assert torch.equal(again.select_action_chunk(img, st, "open drawer", torch.device(DEV)), chunk)
    for p_ in (pol, again):
        p_.model.backbone.engine().close()

    # Trainer: two steps + resume + one step == three steps, bit for bit, with K = 4, L1 and a mask
    data = [_chunk_batch(2, K, seed=s) for s in (1, 2, 3)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1000, eval_steps=1000, seed=1)
    a = _policy(K, "l1", seed=51)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=3, **tkw)).fit()
    b = _policy(K, "l1", seed=51)
    tb = Trainer(b, data[:2], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=2, max_steps=3, **tkw))
    tb.num_training_steps = 3
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-2"
    assert json.loads((ck / "hip_extras.json").read_text())["action_chunk"] == {"chunk_size": K, "n_action_steps": 1, "loss": "l1", "beta": BETA}
    c = _policy(K, "l1", seed=99)      # another initialisation: everything comes from the checkpoint
    tc = Trainer(c, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    tc.num_training_steps = 3
    tc.fit()
    torch.cuda.synchronize()
    assert tc.update_step == 3 and c._opt_state["step"] == 3
    assert torch.equal(a.model._flat, c.model._flat) and torch.equal(a._opt_state["m"], c._opt_state["m"]) and torch.equal(a._opt_state["v"], c._opt_state["v"])
    wrong = _policy(2, "l1", seed=51)
    with pytest.raises(ValueError, match="chunk_size"):
        Trainer(wrong, data, None, TrainingConfig(output_dir=str(tmp_path / "w"), max_steps=1, resume_from=str(ck), **tkw)).fit()
    other = _policy(K, "mse", seed=51)      # another loss than the checkpointed run's: the caller's choice, but said aloud
    to = Trainer(other, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "o"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    to.num_training_steps = 3
    with pytest.warns(UserWarning, match="action loss l1"):
        to.fit()
    for p_ in (a, b, c, other):
        p_.model.backbone.engine().close()
