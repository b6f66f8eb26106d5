"""-m gpu: the LoRA mode of backbone training (fv_train_lora_* in include/fastvla_hip.h; csrc/lora_kernels.hip, csrc/lora_path.inc).

The decoder's matrices stay frozen in the fp32 master, every target matrix runs as W' = W0 + s B A (s = alpha / rank), head and projector train in full.
  1. the projection dW' -> (dA, dB) alone, on random fp32 gradients in every packing at the 0.5B and 7B layer shapes, against float64 products;
  2. commit with B = 0 is the identity; merge then plain commit == adapted commit, bit for bit; the master is never written behind its head | projector front;
  3. one whole step against torch.autograd over the oracle's forward with R(W0 + s B A) as the weight (R = round to bf16, straight-through gradient: the
     rounding the commit applies) and A, B, head, projector as leaves, then the first clip + AdamW step over exactly the trainable tensors;
  4. policy level: a `small` policy with lora_rank=8 overfits one batch, its decoder master does not move, save / load / merge round trips;
  5. two ranks on the one device reproduce the full-batch step, exchanging the trainable buffer only.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, rel_l2  # noqa: E402
from test_gpu_train_unfrozen import GRAD_TOL, _adam_first_update_bound, _inputs, _rig  # noqa: E402  (the unfrozen slice's rig: same weights, same inputs)
from fastvla_hip import FastVLAEngine, FastVLAHipError, arch, lora, weights  # noqa: E402
from oracle import fastvit_hd, head, qwen2, train_unfrozen  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent

LLM_05B = dict(hidden=896, heads=14, kv_heads=2, head_dim=64, inter=4864)
LLM_7B = dict(hidden=3584, heads=28, kv_heads=4, head_dim=128, inter=18944)


def _weight_key(adapter_name):
    """model.layers.3.self_attn.q_proj.lora_A.weight -> model.layers.3.self_attn.q_proj.weight"""
    return adapter_name.replace(".lora_A.weight", ".weight").replace(".lora_B.weight", ".weight")


def _random_adapters(eng, lflat, ltensors, seed, b_std=0.05):
    lora.init_adapters(lflat, ltensors, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    for name, v in lora.adapter_views(lflat, ltensors).items():
        if name.endswith(".lora_B.weight"):
            v.copy_((torch.randn(v.shape, generator=g) * b_std).to(DEV))


# ------------------------------------------------------------------------------------------------------------------ 1. projection, op level
# The ragged decoder shape: the smallest one fv_train_begin admits (hidden and the packed qkv width multiples of 64, inter of 32) at which no adapted matrix is a
# whole number of 128-row projection strips and down_proj is no whole number of 64-column commit tiles:
#   q_proj 192 x 192: one strip and a half          k_proj, v_proj 64 x 192: half a strip          gate_proj, up_proj 352 x 192: two strips and a 96-row one
#   down_proj 192 x 352: 5.5 commit tiles of columns          packed q | k | v: 320 rows, parts at 192 and 256
# (every packed tensor's ROW count is a multiple of 64 at any admitted shape -- hidden, the qkv width and 2 inter all are --, so the commit tile's row edge
# `prow < rows` cannot be false through an engine)
RAGGED_LLM = dict(hidden=192, heads=3, kv_heads=1, head_dim=64, inter=352)
# rank -> what it is there for in the projected mode (lora_project_kernel covers 32 rank indices per launch; lora_delta_tile takes k-pairs, eight k per round):
#   1   odd: the one k-pair is half empty; 31 masked columns of the first launch             24  whole k-pairs, a masked tail of the first launch, three full rounds
#   33  second launch with ONE live rank index (DoRA: dm assembled by two launches); odd       63  second launch one short of full; odd; eight rounds, the last partial
RAGGED_PROJECTED_RANKS = [1, 24, 33, 63]


def _slice_stats(got, ref, dim):
    """the slices of a matrix along `dim` (1: its rows, 0: its columns), each against the RMS slice norm of the reference (||ref||_F / sqrt(slices)) -- a slice
    that happens to be small cannot inflate the ratio.  -> (worst ||got - ref|| of a slice over that RMS, smallest ||ref|| of a slice over that RMS)"""
    ref = ref.double()
    rn = ref.norm(dim=dim)
    rms = float(ref.norm()) / math.sqrt(rn.numel())
    return float((got.double() - ref).norm(dim=dim).max()) / rms, float(rn.min()) / rms


def _projection_case(tag, model, rank, merge=False):
    """fv_train_lora_project on a random fp32 gradient through an engine of this model: dA and dB of all seven matrices against float64 products (1e-5 each), two
    calls bit-identical, head and projector gradients copied.  merge: every rank index of dA (a row) and of dB (a column) is held to the same 1e-5 against the RMS
    slice norm, and fv_train_lora_merge into a copy of the exported master is compared with float64 W0 + s B A (1e-6 per matrix and per output row), every other
    tensor bit-equal.  -> the worst figures"""
    w = weights.init_backbone(model, seed=3)
    eng = FastVLAEngine(model, state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=2, max_text_tokens=8, llm_precision=1)
    eng.load_weights(w)
    eng.train_begin()
    alpha = 2.0 * rank
    eng.train_lora_begin(rank, alpha)
    s = alpha / rank
    _, total, _ = eng.train_layout()
    lt, ltotal = eng.train_lora_layout()
    ref_lt, ref_total = lora.lora_layout(model, rank, None, hidden_dim=64, fusion_dim=64)
    assert lt == ref_lt and ltotal == ref_total       # the host-side mirror IS the library's layout
    g = torch.Generator().manual_seed(11 + rank)
    dW = torch.randn(total, generator=g).to(DEV)
    lflat = torch.zeros(ltotal, device=DEV)
    _random_adapters(eng, lflat, lt, seed=5, b_std=0.3)
    lg = torch.full((ltotal,), float("nan"), device=DEV)
    eng.train_lora_project(dW, lflat, lg)
    torch.cuda.synchronize()
    lg2 = torch.full((ltotal,), float("nan"), device=DEV)
    eng.train_lora_project(dW, lflat, lg2)
    torch.cuda.synchronize()
    assert torch.equal(lg, lg2)                        # fixed summation order
    assert torch.isfinite(lg).all()
    full = eng.train_named_tensors(dW)                 # q / k / v split out of the packed rows, gate / up de-interleaved
    front = lt[16]["offset"]
    assert lt[15]["name"] == "model.mm_projector.2.bias" and torch.equal(lg[:front], dW[:front])   # head and projector gradients move over as they are
    par, got = lora.adapter_views(lflat, lt), lora.adapter_views(lg, lt)
    worst = ("", 0.0)
    out = {"dA": 0.0, "dB": 0.0, "slice": 0.0, "floor": 1e30, "merge": 0.0, "merge_row": 0.0}
    for name in par:
        if not name.endswith(".lora_A.weight"):
            continue
        nb = name.replace(".lora_A.", ".lora_B.")
        d64 = full[_weight_key(name)].double().cpu()
        A, B = par[name].double().cpu(), par[nb].double().cpu()
        for nm, ref, what, dim in ((name, s * (B.t() @ d64), "dA", 1), (nb, s * (d64 @ A.t()), "dB", 0)):
            e = rel_l2(got[nm].cpu(), ref)
            print(f"[lora projection {tag} r={rank}] {nm}: rel_l2 {e:.2e}")
            worst = max(worst, (nm, e), key=lambda t: t[1])
            out[what] = max(out[what], e)
            assert e <= 1e-5, (nm, e)
            if merge:
                es, fl = _slice_stats(got[nm].cpu(), ref, dim)
                out["slice"], out["floor"] = max(out["slice"], es), min(out["floor"], fl)
                assert fl >= 0.1, (nm, fl)            # no rank index is judged against a norm it does not have
                assert es <= 1e-5, (nm, es)
    print(f"[lora projection {tag} r={rank}] worst: {worst[0]} {worst[1]:.2e}")
    if merge:
        flat = torch.zeros(total, device=DEV)
        eng.train_export_params(flat)
        lflat[:front].copy_(flat[:front])              # (the merge mirrors the trainable buffer's head | projector front into the master)
        merged = flat.clone()
        eng.train_lora_merge(merged, lflat)
        torch.cuda.synchronize()
        named0, named1 = eng.train_named_tensors(flat), eng.train_named_tensors(merged)
        adapted = set()
        for name in par:
            if name.endswith(".lora_A.weight"):
                k = _weight_key(name)
                adapted.add(k)
                ref = named0[k].double().cpu() + s * (par[name.replace(".lora_A.", ".lora_B.")].double().cpu() @ par[name].double().cpu())
                e = rel_l2(named1[k].cpu(), ref)
                er, fl = _slice_stats(named1[k].cpu(), ref, 1)
                print(f"[lora merge {tag} r={rank}] {k}: rel_l2 {e:.2e}, worst row {er:.2e}")
                out["merge"], out["merge_row"], out["floor"] = max(out["merge"], e), max(out["merge_row"], er), min(out["floor"], fl)
                assert fl >= 0.1, (k, fl)
                assert e <= 1e-6 and er <= 1e-6, (k, e, er)
        assert len(adapted) == 7 * model.llm.layers
        for k in named0:
            if k not in adapted:
                assert torch.equal(named0[k], named1[k]), k
        # the adapted commit's bf16 rows (lora_commit_kernel<0>, partial tile of columns included), read back: the merged master rounded to bf16, bit for bit
        eng.train_lora_commit(flat, lflat)
        back = torch.zeros(total, device=DEV)
        eng.train_export_params(back)
        torch.cuda.synchronize()
        named_b = eng.train_named_tensors(back)
        for k in adapted:
            assert torch.equal(named_b[k], named1[k].to(torch.bfloat16).float()), k
        print(f"[lora projection {tag} r={rank}] worst slice {out['slice']:.2e}; merged master {out['merge']:.2e}, row {out['merge_row']:.2e}; "
              f"smallest reference slice / RMS {out['floor']:.2f}")
    eng.close()
    return out


@pytest.mark.parametrize("shape", ["0.5b", "7b"])
@pytest.mark.parametrize("rank", [4, 16, 64])
def test_projection_matches_float64_products(shape, rank):
    """rel-L2 <= 1e-5 per output matrix.  Derived, not measured: an fp32 sum of K random terms in any order errs by about sqrt(K) 2^-24 -- 8e-6 at the largest
    contraction here (K = 18944) -- and an operand rounded to bf16 / fp16 lands at 2e-4 or worse."""
    dims = LLM_05B if shape == "0.5b" else LLM_7B
    model = arch.ModelConfig("lora-" + shape, arch.LLMConfig(layers=1, vocab=512, **dims), arch.preset("tiny").tower)
    _projection_case(shape, model, rank)


@pytest.mark.parametrize("rank", RAGGED_PROJECTED_RANKS)
def test_projection_and_merge_at_the_ragged_shape(rank):
    """The projection and the merge at the ragged layer (RAGGED_LLM: partial strips, a partial commit tile of columns) and at the ranks of RAGGED_PROJECTED_RANKS
    (odd ranks, masked tails, a partial second launch).  The bars are those of test_projection_matches_float64_products (1e-5 per matrix; the contractions here
    are at most 352 long) and of test_commit_identity_and_merge_equals_commit (1e-6 for the merged master); every rank index of dA and dB and every output row
    of a merged matrix is held to its matrix's bar against the RMS slice norm of the reference, none of which is below a tenth of that RMS (asserted; the
    smallest is 0.53).  Measured on the MI355X, worst over the four ranks: dA 1.2e-7, dB 3.5e-7 (down_proj.lora_B), slice 4.1e-7,
    merged master 1.5e-7, merged row 2.1e-7."""
    model = arch.ModelConfig("lora-ragged", arch.LLMConfig(layers=1, vocab=512, **RAGGED_LLM), arch.preset("tiny").tower)
    _projection_case("ragged", model, rank, merge=True)


# ------------------------------------------------------------------------------------------------------------------ 2. commit / merge
def _commit_merge_case(model, rank):
    """commit with B = 0 is the identity; random B: adapted commit == merge into a copy + plain commit, bit for bit in llm_pooled and in the whole gradient of a
    step (the bf16 rows, the transposed fp16 copies); the merged master against float64 at 1e-6; nothing else of the master is written"""
    B, T = 3, 16
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, 64, B, T)
    tower_out, ids, mask, states, targets = _inputs(model, B, T, 42)
    with torch.no_grad():
        tok = fastvit_hd.projector_forward(w, tower_out.float()).to(DEV)
    alpha = 2.0 * rank
    s = alpha / rank
    eng.train_commit(flat)
    pooled0 = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    eng.train_lora_begin(rank, alpha)
    with pytest.raises(FastVLAHipError):
        eng.train_tower_begin()                        # tower adapters do not exist: the two modes exclude each other
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    lora.init_adapters(lflat, lt, seed=1)              # B = 0
    master0 = flat.clone()
    eng.train_lora_commit(flat, lflat)
    pooled_id = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    torch.cuda.synchronize()
    assert torch.equal(pooled_id, pooled0)
    assert torch.equal(flat, master0)
    # random B: adapted commit on the original master == merge into a copy + plain commit
    _random_adapters(eng, lflat, lt, seed=2)
    eng.train_lora_commit(flat, lflat)
    pooled_lora = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    ws = eng.train_workspace(B, T)
    _, _, g_lora = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=torch.zeros_like(flat))
    lg = torch.zeros(ltotal, device=DEV)
    eng.train_lora_project(g_lora, lflat, lg)
    torch.cuda.synchronize()
    assert torch.equal(flat, master0)                  # neither commit nor project writes W0
    assert float((pooled_lora - pooled0).abs().max()) > 0
    merged = flat.clone()
    eng.train_lora_merge(merged, lflat)
    eng.train_commit(merged)
    pooled_merged = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    _, _, g_merged = eng.train_forward_backward(merged, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=torch.zeros_like(flat))
    torch.cuda.synchronize()
    assert torch.equal(pooled_merged, pooled_lora)
    assert torch.equal(g_merged, g_lora)               # ... the transposed dgrad copies included
    named0, named1 = eng.train_named_tensors(master0), eng.train_named_tensors(merged)
    par = lora.adapter_views(lflat, lt)
    adapted = set()
    for name in par:
        if name.endswith(".lora_A.weight"):
            k = _weight_key(name)
            adapted.add(k)
            ref = named0[k].double().cpu() + s * (par[name.replace(".lora_A.", ".lora_B.")].double().cpu() @ par[name].double().cpu())
            e = rel_l2(named1[k].cpu(), ref)
            assert e <= 1e-6, (k, e)
    assert len(adapted) == 7 * model.llm.layers
    for k in named0:
        if k not in adapted:
            assert torch.equal(named0[k], named1[k]), k
    eng.close()


def test_commit_identity_and_merge_equals_commit():
    _commit_merge_case(arch.preset("small"), 16)


def test_commit_and_merge_agree_at_the_ragged_shape():
    """_commit_merge_case on two ragged layers (RAGGED_LLM) at rank 33, odd and with a one-index second round of k: merge + plain commit must give the same bits
    as the adapted commit in llm_pooled and in every gradient of a step -- the only check that reaches the transposed fp16 copies and the fp16 row copies
    lora_commit_kernel<0> writes at a partial tile of columns (down_proj: 5.5 tiles).  It runs the decoder at this geometry: the ragged case of
    test_unfrozen_step_matches_autograd is its control."""
    _commit_merge_case(arch.ModelConfig("lora-ragged-2", arch.LLMConfig(layers=2, vocab=512, **RAGGED_LLM), arch.preset("tiny").tower), 33)


# ------------------------------------------------------------------------------------------------------------------ 3. one step against autograd
def _lora_oracle(w, hp, par, s, tower_out, ids, mask, states, targets, lc, rounded=True):
    """autograd over projector -> spliced decoder -> head -> MSE with W' = R(W0 + s B A) on every adapted matrix; leaves: A, B, head, projector"""
    leaves = {k: v.detach().clone().float().cpu().requires_grad_(True) for k, v in par.items()}
    q = dict(w)
    for k in w:
        if k.startswith("model.mm_projector."):
            leaves[k] = w[k].detach().clone().float().requires_grad_(True)
            q[k] = leaves[k]
    for name in par:
        if name.endswith(".lora_A.weight"):
            k = _weight_key(name)
            merged = w[k].float() + s * (leaves[name.replace(".lora_A.", ".lora_B.")] @ leaves[name])
            q[k] = fastvit_hd._r(merged) if rounded else merged
    hl = {k: v.detach().clone().float().requires_grad_(True) for k, v in hp.items()}
    tok = fastvit_hd.projector_forward(q, tower_out.float())
    pooled = qwen2.llm_pooled(q, ids, mask, lc, image_tokens=tok, splice=True)
    pred = head.head_forward(hl, pooled, states)
    loss = F.mse_loss(pred, targets)
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads.update({"head." + k: v.grad for k, v in hl.items()})
    params = {k: v.detach() for k, v in leaves.items()}
    params.update({"head." + k: v.detach() for k, v in hl.items()})
    return {"loss": loss.detach(), "pred": pred.detach(), "grads": grads, "params": params}


def _trainable_named(lflat, lt):
    out = {}
    for t in lt:
        v = lflat[t["offset"]: t["offset"] + t["numel"]]
        v = v.view(t["rows"], t["cols"]) if t["rows"] > 1 else v
        out[("head." if t["bucket"] == 0 else "") + t["name"]] = v
    return out


@pytest.mark.parametrize("name,llm,B,T,hd,rank,targets", [
    ("small", None, 3, 16, 64, 16, None),
    ("small", None, 3, 16, 64, 4, ("q_proj", "v_proj")),
    ("0.5b-width-4-layers", arch.LLMConfig(hidden=896, layers=4, heads=14, kv_heads=2, head_dim=64, inter=4864, vocab=8192), 4, 32, 128, 16, None),
    ("7b-width-2-layers", arch.LLMConfig(hidden=3584, layers=2, heads=28, kv_heads=4, head_dim=128, inter=18944, vocab=4096), 2, 16, 128, 16, None),
    # two ragged layers (RAGGED_LLM: partial strips and commit tiles, GQA group 3 on one kv head) at a rank with a masked tail; control: the unfrozen step's ragged case
    ("ragged-2-layers", arch.LLMConfig(layers=2, vocab=512, **RAGGED_LLM), 3, 16, 64, 24, None),
])
def test_lora_step_matches_autograd(name, llm, B, T, hd, rank, targets):
    model = arch.preset("small") if llm is None else arch.ModelConfig(name, llm, arch.preset("tiny").tower)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, hd, B, T)
    tower_out, ids, mask, states, targets_ = _inputs(model, B, T, 42)
    alpha = 2.0 * rank
    s = alpha / rank
    eng.train_lora_begin(rank, alpha, targets)
    lt, ltotal = eng.train_lora_layout()
    want = lora.parse_targets(targets)
    adapters = [t["name"] for t in lt if ".lora_" in t["name"]]
    assert len(adapters) == 2 * len(want) * model.llm.layers           # non-target matrices get no adapter entries
    assert all(n.split(".")[4] in want for n in adapters)
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    master0 = flat.clone()
    eng.train_lora_commit(flat, lflat)
    ws = eng.train_workspace(B, T)
    full_g = torch.zeros_like(flat)
    lg = torch.zeros(ltotal, device=DEV)

    def run():
        act, loss, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False, flat_grads=full_g)
        eng.train_lora_project(full_g, lflat, lg)
        torch.cuda.synchronize()
        return act.clone(), loss.clone(), lg.clone()

    act, loss, grads = run()
    assert torch.equal(flat, master0)
    par = {k: v.clone() for k, v in lora.adapter_views(lflat, lt).items()}
    ref = _lora_oracle(w, hp, par, s, tower_out, ids, mask, states, targets_, lc, rounded=True)
    ra, rl = rel_l2(act.cpu(), ref["pred"]), abs(float(loss) - float(ref["loss"])) / float(ref["loss"])

    def grad_errors(g):
        got = _trainable_named(g / eng.train_loss_scale(), lt)
        assert set(got) == set(ref["grads"]), sorted(set(got) ^ set(ref["grads"]))[:8]
        return sorted(((rel_l2(v.cpu(), ref["grads"][k]), k) for k, v in got.items() if float(ref["grads"][k].norm()) > 1e-12), reverse=True)

    errs = grad_errors(grads)
    print(f"[lora {name} r={rank} targets={','.join(want)}] actions rel_l2={ra:.2e} loss rel={rl:.2e}; worst gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:4])
          + f" ({len(errs)} tensors)")
    # for the record only: the same comparison against the oracle WITHOUT the commit's rounding of W0 + s B A
    raw = _lora_oracle(w, hp, par, s, tower_out, ids, mask, states, targets_, lc, rounded=False)
    print(f"[lora {name} r={rank}] against the unrounded oracle: actions rel_l2={rel_l2(act.cpu(), raw['pred']):.2e} "
          f"loss rel={abs(float(loss) - float(raw['loss'])) / float(raw['loss']):.2e}")
    # ... and the most exact backward (split-bf16 dgrad operands, two passes), as the unfrozen slice's test prints it
    eng.train_set_options(grad_split=1)
    _, _, g1 = run()
    e1 = grad_errors(g1)
    print(f"[lora {name} r={rank}] grad_split=1: worst gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in e1[:3]))
    eng.train_set_options()
    eng.train_lora_commit(flat, lflat)      # (the switch rebuilt the transposed copies from the library's weights: same images)
    act2, loss2, grads2 = run()
    assert torch.equal(act2, act) and torch.equal(loss2, loss) and torch.equal(grads2, grads)    # bit-identical repeat
    assert ra <= 1e-3 and rl <= 1e-3
    for e, k in errs:
        assert e <= GRAD_TOL, f"gradient of {k}: rel_l2 {e:.3e} > {GRAD_TOL}"
    # first clip + AdamW step over exactly the trainable tensors (clip_grad_norm_ over requires_grad parameters)
    m, v, norm = torch.zeros_like(lflat), torch.zeros_like(lflat), torch.zeros(1, device=DEV)
    new = lflat.clone()
    eng.adamw_step(new, grads, m, v, 1, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, grad_norm_out=norm, grad_scale=1.0 / eng.train_loss_scale())
    torch.cuda.synchronize()
    ref_new, ref_norm = train_unfrozen.adamw_clip_step(ref["params"], ref["grads"], lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    assert abs(float(norm) - float(ref_norm)) <= 2e-3 * float(ref_norm)
    got_new = _trainable_named(new, lt)
    coef = min(1.0, 1.0 / (float(ref_norm) + 1e-6))
    for k, r in ref_new.items():
        p0 = ref["params"][k]
        du, dr = got_new[k].cpu() - p0.reshape(got_new[k].shape), (r - p0).reshape(got_new[k].shape)
        big = (ref["grads"][k].reshape(du.shape) * coef).abs() > 1e-6      # (entries with a gradient near Adam's eps move by lr * noise: bounded only)
        assert float(du.abs().max()) <= _adam_first_update_bound(float(p0.abs().max())), k
        if big.any():
            bad = float(((du - dr).abs()[big] > 0.05 * 1e-3 + 1e-2 * dr.abs()[big]).float().mean())
            assert bad <= 5e-3, (k, bad)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4. policy level
def test_policy_level_lora_training_overfits_one_batch_and_round_trips(tmp_path):
    """FastVLAPolicy.enable_backbone_training(lora_rank=8) + fused_train_step on one fixed batch of the `small` policy (the batch, learning rate and criterion
    of the unfrozen slice's policy-level test; its 16 steps suffice: 0.90 -> 0.22)."""
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    from vla_fastvlm.utils import load_policy_from_checkpoint, save_policy_checkpoint
    from vla_fastvlm.utils.checkpoint import LORA_FILE
    torch.manual_seed(5)
    cfg = FastVLAConfig(vlm_model_name="synthetic:small:41", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
    g = torch.Generator().manual_seed(6)
    B = 4
    batch = {"images": torch.rand(B, 3, 96, 128, generator=g).to(DEV), "states": torch.randn(B, 14, generator=g).to(DEV),
             "actions": torch.randn(B, 14, generator=g).to(DEV), "tasks": ["pick up the red cube", "open the drawer", "push", "pick up the red cube"]}
    pol = FastVLAPolicy(cfg).to(DEV)
    pol.train()
    with pytest.raises(ValueError):
        pol.enable_backbone_training(tower=True, lora_rank=8)
    st = pol.enable_backbone_training(lora_rank=8)
    assert st.lora == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS)} and pol.model.backbone.splice_image_tokens is True
    assert st.m.numel() == st.v.numel() == st.lflat.numel() == st.lora_total < st.flat.numel() // 2       # moments over the trainable buffer only
    master0 = st.flat.clone()
    a0 = {k: v.clone() for k, v in lora.adapter_views(st.lflat, st.lora_tensors).items()}
    assert all(float(v.abs().max()) == 0.0 for k, v in a0.items() if k.endswith("lora_B.weight"))          # PEFT's start: B = 0 ...
    assert all(float(v.abs().max()) <= 1.0 / math.sqrt(v.shape[1]) and float(v.std()) > 0 for k, v in a0.items() if k.endswith("lora_A.weight"))
    losses = []
    for i in range(16):
        out = pol.fused_train_step(batch, lr=2e-3, weight_decay=0.0)
        losses.append(float(out["loss"]))
    torch.cuda.synchronize()
    print("[lora policy] loss over 16 steps on one batch:", " ".join(f"{x:.4f}" for x in losses))
    assert all(map(math.isfinite, losses)) and losses[-1] < 0.6 * losses[0]
    assert torch.equal(st.flat[st.front:], master0[st.front:])                  # the decoder master did not move ...
    assert torch.equal(st.flat[: st.front], st.lflat[: st.front])               # ... and its head | projector front mirrors the trained one
    a1 = lora.adapter_views(st.lflat, st.lora_tensors)
    assert all(not torch.equal(a0[k], a1[k]) for k in a0)                        # every adapter trained
    pol.eval()
    with torch.no_grad():
        a = pol(batch["images"], batch["states"], batch["tasks"]).clone()
    assert float(((a - batch["actions"]) ** 2).mean()) < 0.7 * losses[0]
    # adapters + config in a file of their own beside the reference's two; policy_state_dict.pt keeps exactly the reference's keys
    out_dir = save_policy_checkpoint(pol, tmp_path / "lora")
    sd = torch.load(out_dir / "policy_state_dict.pt", map_location="cpu")
    plain = FastVLAPolicy(cfg)
    assert set(sd) == set(plain.state_dict())
    ex = json.loads((out_dir / "hip_extras.json").read_text())
    assert ex["lora"] == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS), "file": LORA_FILE} and ex["splice_image_tokens"] is True
    assert (out_dir / LORA_FILE).stat().st_size < 0.5 * 4 * st.flat.numel()
    again = load_policy_from_checkpoint(str(out_dir)).to(DEV)
    with torch.no_grad():
        a2 = again(batch["images"], batch["states"], batch["tasks"])
    torch.cuda.synchronize()
    assert torch.equal(a2, a)                                                    # select_action's forward on the adapted weights, bit for bit
    sel = again.select_action(batch["images"][0], batch["states"][0], batch["tasks"][0], torch.device(DEV))
    sel0 = pol.select_action(batch["images"][0], batch["states"][0], batch["tasks"][0], torch.device(DEV))
    assert torch.equal(sel, sel0)
    # a directory whose extras name adapters that are not there does not load
    broken = tmp_path / "broken"
    save_policy_checkpoint(pol, broken)
    (broken / LORA_FILE).unlink()
    with pytest.raises(FileNotFoundError):
        load_policy_from_checkpoint(str(broken))
    # gradient accumulation: two half batches == the full batch, on the trainable buffer
    pa, pb = FastVLAPolicy(cfg).to(DEV), FastVLAPolicy(cfg).to(DEV)
    for p_ in (pa, pb):
        p_.train()
    sa, sb = pa.enable_backbone_training(lora_rank=8), pb.enable_backbone_training(lora_rank=8)
    for s_ in (sa, sb):
        s_.lflat.copy_(st.lflat)
        s_.commit()
    pa.fused_train_step(batch, lr=1e-3)
    half = lambda lo, hi: {k: v[lo:hi] for k, v in batch.items()}   # noqa: E731
    pb.fused_train_step(half(0, 2), lr=1e-3, grad_accum_steps=2)
    pb.fused_train_step(half(2, 4), lr=1e-3, grad_accum_steps=2)
    torch.cuda.synchronize()
    assert sb.acc.numel() == sb.lflat.numel()
    assert rel_l2((sb.acc / 2).cpu(), sa.lg.cpu()) <= 2e-3
    # merge_lora(): the adapters fold into the master; the backbone export writes a plain reference-keyed checkpoint that a fresh policy loads
    pol.merge_lora()
    with pytest.raises(ValueError):
        save_policy_checkpoint(pol, tmp_path / "nope")                           # the merged master must travel: adapters alone no longer describe the model
    with torch.no_grad():
        am = pol(batch["images"], batch["states"], batch["tasks"])
    assert torch.equal(am, a)                                                    # merging changes nothing the model computes
    assert not torch.equal(st.flat[st.front:], master0[st.front:])
    merged_dir = save_policy_checkpoint(pol, tmp_path / "merged", include_backbone=True)
    assert not (merged_dir / LORA_FILE).exists() and "lora" not in json.loads((merged_dir / "hip_extras.json").read_text())
    sdm = torch.load(merged_dir / "policy_state_dict.pt", map_location="cpu")
    k0 = "model.backbone.model.model.layers.0.mlp.down_proj.weight"
    assert torch.equal(sdm[k0], st.named_backbone_tensors()["model.layers.0.mlp.down_proj.weight"].cpu())
    fresh = load_policy_from_checkpoint(str(merged_dir)).to(DEV)
    assert fresh._unfrozen is None
    with torch.no_grad():
        a3 = fresh(batch["images"], batch["states"], batch["tasks"])
    torch.cuda.synchronize()
    e = rel_l2(a3.cpu(), a.cpu())
    print(f"[lora policy] merged plain checkpoint vs the adapted policy: actions rel_l2 {e:.2e}")
    assert e <= 1e-5
    for p_ in (pol, again, pa, pb, fresh):
        p_.model.backbone.engine().close()


# ------------------------------------------------------------------------------------------------------------------ 5. two ranks, device tensors
def test_two_rank_lora_step_equals_the_full_batch_step(tmp_path):
    """Two fresh rank processes on the one GPU (gloo, as the unfrozen slice's two-rank test), each on half of one fixed batch: what they exchange is the
    trainable buffer -- one collective -- and the reduced gradient, its norm and the loss reproduce the full-batch LoRA step."""
    worker = str(ROOT / "tools" / "lora_dp_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    one = tmp_path / "w1"
    one.mkdir()
    r = subprocess.run([sys.executable, worker, "--out", str(one)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    two = tmp_path / "w2"
    two.mkdir()
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, worker, "--out", str(two)], env=dict(env, RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                                                                   MASTER_PORT=str(port)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in range(2)]
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    full = torch.load(one / "rank0.pt")
    r0, r1 = torch.load(two / "rank0.pt"), torch.load(two / "rank1.pt")
    assert r0["world"] == 2
    for r_ in (full, r0, r1):
        assert r_["payload"] == r_["trainable"] == r_["moments"] < r_["full"] // 2 and r_["bucketed"] == [] and r_["master_unchanged"]
    assert torch.equal(r0["grads"], r1["grads"]) and torch.equal(r0["lflat"], r1["lflat"])      # replicas stay identical
    e = rel_l2(r0["grads"], full["grads"])
    print(f"[lora dp2 vs full batch] reduced gradient rel_l2 {e:.2e}; grad norm {r0['grad_norm']:.4f} vs {full['grad_norm']:.4f}; payload {r0['payload']} of {r0['full']} floats")
    assert e <= 2e-3 and abs(r0["grad_norm"] - full["grad_norm"]) <= 2e-3 * full["grad_norm"]
    assert abs(0.5 * (r0["loss"] + r1["loss"]) - full["loss"]) <= 1e-4 * abs(full["loss"])


def test_trainer_fit_in_lora_mode_saves_adapters_and_resumes(tmp_path):
    """`Trainer.fit()` over several batches in LoRA mode (the route of the unfrozen slice's trainer test): its checkpoints carry the head under the reference's keys,
    the adapters in their own file and the moments of the TRAINABLE buffer -- not the VLM --, and a run resumed from one, on a policy that was never told about
    LoRA, continues bit for bit where the uninterrupted run is."""
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils.checkpoint import LORA_FILE
    g = torch.Generator().manual_seed(8)

    def mk(B):
        return {"images": torch.rand(B, 3, 96, 128, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, 14, generator=g),
                "tasks": ["pick up the red cube", "open the drawer", "push"][:B]}

    data = [mk(3), mk(3), mk(3), mk(3)]
    cfg = FastVLAConfig(vlm_model_name="synthetic:small:43", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1000, eval_steps=1000, seed=1)
    lcfg = {"rank": 4, "alpha": 8.0, "targets": ["q_proj", "v_proj", "down_proj"]}

    def fresh(enable=True):
        torch.manual_seed(7)
        p = FastVLAPolicy(cfg).to(DEV)
        if enable:
            p.enable_backbone_training(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"])
        return p

    a = fresh()
    master0 = a._unfrozen.flat.clone()
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=4, **tkw)).fit()
    b = fresh()
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=4, **tkw))
    tb.num_training_steps = 4
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    sd = torch.load(ck / "policy_state_dict.pt", map_location="cpu")
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert not any(k.startswith("model.backbone.model.") for k in sd)          # the frozen VLM does not travel with a LoRA run
    assert json.loads((ck / "hip_extras.json").read_text()) == {"splice_image_tokens": True, "train_backbone": True, "train_tower": False, "lora": {**lcfg, "file": LORA_FILE}}
    ad = torch.load(ck / LORA_FILE, map_location="cpu")
    assert ad["config"] == lcfg and "model.mm_projector.2.weight" in ad["tensors"] and "model.layers.2.mlp.down_proj.lora_B.weight" in ad["tensors"]
    assert float(ad["tensors"]["model.layers.0.self_attn.q_proj.lora_B.weight"].abs().max()) > 0
    assert opt["lora"] == lcfg and opt["m"].numel() == opt["flat"].numel() == b._unfrozen.lflat.numel() and int(opt["step"]) == 3
    c = fresh(enable=False)                                                        # what the run trains comes back from the checkpoint
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=4, resume_from=str(ck), **tkw))
    tc.num_training_steps = 4
    tc.fit()
    torch.cuda.synchronize()
    assert tc.global_step == 4 and c._unfrozen.step_count == 4 and c._unfrozen.lora == lcfg
    assert torch.equal(c._unfrozen.lflat, a._unfrozen.lflat) and torch.equal(c._unfrozen.m, a._unfrozen.m)     # the resumed run IS the uninterrupted one
    front = a._unfrozen.front
    assert torch.equal(a._unfrozen.flat[front:], master0[front:]) and torch.equal(c._unfrozen.flat, a._unfrozen.flat)
    for p_ in (a, b, c):
        p_.model.backbone.engine().close()
