"""-m gpu: the DoRA and rsLoRA variants of LoRA mode (fv_train_lora_begin_ex, fv_train_lora_init_magnitude in include/fastvla_hip.h; csrc/lora_kernels.hip,
csrc/lora_path.inc).

DoRA: every adapted matrix runs as W' = diag(m / n) V, V = W0 + s B A, n its row norms (a constant in the backward, as in PEFT), m a trained magnitude per row.
rsLoRA: s = alpha / sqrt(rank).  The plain LoRA mode (tests/test_gpu_lora.py) supplies the rigs, the shapes and the bars.
  1. row norms, dA, dB, dm alone, on random fp32 gradients in every packing at the 0.5B and 7B layer shapes, against float64;
  2. at initialisation (B = 0, m = n) the adapted commit is the plain commit bit for bit; random B and m: merge against float64, merge + plain commit == adapted
     commit bit for bit, re-initialised magnitudes give c == 1;
  3. one whole step against torch.autograd with W' = R(diag(m / n.detach()) (W0 + s B A)) and A, B, m, head, projector as leaves, then clip + AdamW; one rsLoRA
     case without DoRA through the same oracle, projected and direct;
  4. refusals; 5. policy level: overfit, save / load, merge, Trainer resume, two ranks.
"""
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, rel_l2  # noqa: E402
from test_gpu_lora import LLM_05B, LLM_7B, RAGGED_LLM, RAGGED_PROJECTED_RANKS, _random_adapters, _slice_stats, _trainable_named  # noqa: E402
from test_gpu_train_unfrozen import GRAD_TOL, _inputs, _rig  # noqa: E402
from fastvla_hip import FastVLAEngine, FastVLAHipError, _lib, arch, lora, weights  # noqa: E402
from oracle import fastvit_hd, head, qwen2, train_unfrozen  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
MAG = ".lora_magnitude_vector.weight"


def _weight_key(name):
    for suffix in (".lora_A.weight", ".lora_B.weight", MAG):
        name = name.replace(suffix, ".weight")
    return name


def _targets_of(par):
    """adapter prefix ("model.layers.0.self_attn.q_proj") of every adapted matrix"""
    return [k[: -len(".lora_A.weight")] for k in par if k.endswith(".lora_A.weight")]


def _random_magnitudes(eng, flat, lflat, lt, seed):
    """m <- n (fv_train_lora_init_magnitude, for the A, B in lflat) times a random factor in [0.5, 1.5): positive, and nowhere equal to n.  -> n per tensor"""
    eng.train_lora_init_magnitude(flat, lflat)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(seed)
    norms = {}
    for name, v in lora.adapter_views(lflat, lt).items():
        if name.endswith(MAG):
            norms[name] = v.clone().reshape(-1)
            f = 0.5 + torch.rand(v.shape, generator=g)
            f[(f - 1.0).abs() < 1e-3] = 1.25
            v.mul_(f.to(DEV))
    return norms


# ------------------------------------------------------------------------------------------------------------------ 1. norms and projection, op level
def _dora_op_case(shape, model, rank, merge=False):
    """row norms, dA, dB and dm of every adapted matrix of this model against float64 (1e-5 each), two calls bit-identical, head and projector gradients copied.
    merge: every rank index of dA (a row) and of dB (a column) is held to the same 1e-5 against the RMS slice norm, and fv_train_lora_merge into a copy of the
    master is compared with float64 diag(m / n) (W0 + s B A): 1e-5 per matrix and row by row.  -> the worst figures"""
    w = weights.init_backbone(model, seed=3)
    eng = FastVLAEngine(model, state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=2, max_text_tokens=8, llm_precision=1)
    eng.load_weights(w)
    eng.train_begin()
    alpha = 2.0 * rank
    eng.train_lora_begin(rank, alpha, dora=True)
    s = alpha / rank
    _, total, _ = eng.train_layout()
    flat = torch.zeros(total, device=DEV)
    eng.train_export_params(flat)
    lt, ltotal = eng.train_lora_layout()
    ref_lt, ref_total = lora.lora_layout(model, rank, None, hidden_dim=64, fusion_dim=64, dora=True)
    assert lt == ref_lt and ltotal == ref_total       # the host-side mirror IS the library's layout
    assert lt[15]["name"] == "model.mm_projector.2.bias" and lt[16]["name"].endswith(".lora_A.weight")
    g = torch.Generator().manual_seed(11 + rank)
    dW = torch.randn(total, generator=g).to(DEV)
    lflat = torch.zeros(ltotal, device=DEV)
    lflat[: lt[16]["offset"]].copy_(flat[: lt[16]["offset"]])      # (the commit mirrors the trainable buffer's head | projector front into the master)
    _random_adapters(eng, lflat, lt, seed=5, b_std=0.3)
    lg = torch.full((ltotal,), float("nan"), device=DEV)
    with pytest.raises(FastVLAHipError):
        eng.train_lora_project(dW, lflat, lg)          # no commit has run: there are no norms to use
    norms = _random_magnitudes(eng, flat, lflat, lt, seed=21)
    master0 = flat.clone()
    eng.train_lora_commit(flat, lflat)
    eng.train_lora_project(dW, lflat, lg)
    torch.cuda.synchronize()
    lg2 = torch.full((ltotal,), float("nan"), device=DEV)
    eng.train_lora_commit(flat, lflat)
    eng.train_lora_project(dW, lflat, lg2)
    torch.cuda.synchronize()
    assert torch.equal(flat, master0)
    used = torch.zeros(ltotal, dtype=torch.bool, device=DEV)
    for t in lt:
        used[t["offset"]: t["offset"] + t["numel"]] = True
    assert torch.equal(lg[used], lg2[used])            # fixed summation order
    assert torch.isfinite(lg[used]).all()
    front = lt[16]["offset"]
    assert torch.equal(lg[:front], dW[:front])         # head and projector gradients move over as they are
    full, w0 = eng.train_named_tensors(dW), eng.train_named_tensors(flat)
    par, got = lora.adapter_views(lflat, lt), lora.adapter_views(lg, lt)
    worst = {"n": 0.0, "dA": 0.0, "dB": 0.0, "dm": 0.0}
    pres = _targets_of(par)
    assert len(pres) == 7
    for pre in pres:
        k = pre + ".weight"
        G, W0 = full[k].double().cpu(), w0[k].double().cpu()
        A, B, m = par[pre + ".lora_A.weight"].double().cpu(), par[pre + ".lora_B.weight"].double().cpu(), par[pre + MAG].double().cpu().reshape(-1)
        V = W0 + s * (B @ A)
        n = V.norm(dim=1)
        c = m / n
        assert float((m / n - 1).abs().min()) > 1e-4    # m is NOT n: c does real work
        refs = {"n": (norms[pre + MAG].cpu(), n), "dA": (got[pre + ".lora_A.weight"].cpu(), s * (B.t() @ (c[:, None] * G))),
                "dB": (got[pre + ".lora_B.weight"].cpu(), s * ((c[:, None] * G) @ A.t())), "dm": (got[pre + MAG].cpu().reshape(-1), (G * V).sum(1) / n)}
        for what, (have, ref) in refs.items():
            e = rel_l2(have, ref)
            print(f"[dora op {shape} r={rank}] {pre} {what}: rel_l2 {e:.2e}")
            worst[what] = max(worst[what], e)
            assert e <= 1e-5, (pre, what, e)
            if merge and what in ("dA", "dB"):
                es, fl = _slice_stats(have, ref, 1 if what == "dA" else 0)
                worst["slice"], worst["floor"] = max(worst.get("slice", 0.0), es), min(worst.get("floor", 1e30), fl)
                assert fl >= 0.1, (pre, what, fl)      # no rank index is judged against a norm it does not have
                assert es <= 1e-5, (pre, what, es)
    print(f"[dora op {shape} r={rank}] worst: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if merge:
        merged = flat.clone()
        eng.train_lora_merge(merged, lflat)
        torch.cuda.synchronize()
        named1 = eng.train_named_tensors(merged)
        for pre in pres:
            k = pre + ".weight"
            V = w0[k].double().cpu() + s * (par[pre + ".lora_B.weight"].double().cpu() @ par[pre + ".lora_A.weight"].double().cpu())
            ref = (par[pre + MAG].double().cpu().reshape(-1) / V.norm(dim=1))[:, None] * V
            e = rel_l2(named1[k].cpu(), ref)
            rows = float(((named1[k].double().cpu() - ref).norm(dim=1) / ref.norm(dim=1)).max())     # row by row, each against its own norm ...
            er, fl = _slice_stats(named1[k].cpu(), ref, 1)                                             # ... and against the RMS row norm
            print(f"[dora merge {shape} r={rank}] {k}: rel_l2 {e:.2e}, worst row {max(rows, er):.2e}")
            worst["merge"], worst["merge_row"] = max(worst.get("merge", 0.0), e), max(worst.get("merge_row", 0.0), rows, er)
            worst["floor"] = min(worst["floor"], fl)
            assert fl >= 0.1, (k, fl)
            assert e <= 1e-5 and rows <= 1e-5 and er <= 1e-5, (k, e, rows, er)
        for k in w0:
            if k not in {pre + ".weight" for pre in pres}:
                assert torch.equal(w0[k], named1[k]), k
        # the adapted commit's bf16 rows (lora_commit_kernel<0, 1>, partial tile of columns included), read back: the merged master rounded to bf16, bit for bit
        eng.train_lora_commit(flat, lflat)
        back = torch.zeros(total, device=DEV)
        eng.train_export_params(back)
        torch.cuda.synchronize()
        named_b = eng.train_named_tensors(back)
        for pre in pres:
            assert torch.equal(named_b[pre + ".weight"], named1[pre + ".weight"].to(torch.bfloat16).float()), pre
        print(f"[dora op {shape} r={rank}] worst slice {worst['slice']:.2e}; merged master {worst['merge']:.2e}, row {worst['merge_row']:.2e}; "
              f"smallest reference slice / RMS {worst['floor']:.2f}")
    eng.close()
    return worst


@pytest.mark.parametrize("shape", ["0.5b", "7b"])
@pytest.mark.parametrize("rank", [4, 16, 64])
def test_norms_and_projection_match_float64(shape, rank):
    """rel-L2 <= 1e-5 for n, dA, dB and dm of every adapted matrix: the project's derived bar for fp32 sums (an fp32 sum of K terms in any order errs by about
    sqrt(K) 2^-24: 8e-6 at K = 18944; lane-partial sums, which both new reductions use, sit near 5e-7).  Two calls are bit-identical; head and projector
    gradients are copied.  Measured on the MI355X, worst over the six cases: n 5.6e-8, dA 2.5e-7, dB 2.5e-6, dm 1.8e-6
    (dB and dm carry the K-long fmaf chain of the dW' . A^T accumulator: both worst cases are down_proj at the 7B shape, K = 18944)."""
    dims = LLM_05B if shape == "0.5b" else LLM_7B
    _dora_op_case(shape, arch.ModelConfig("dora-" + shape, arch.LLMConfig(layers=1, vocab=512, **dims), arch.preset("tiny").tower), rank)


@pytest.mark.parametrize("rank", RAGGED_PROJECTED_RANKS)
def test_norms_projection_and_merge_at_the_ragged_shape(rank):
    """_dora_op_case at the ragged layer (RAGGED_LLM in test_gpu_lora.py: partial strips, a partial commit tile of columns) and at the ranks of
    RAGGED_PROJECTED_RANKS: at 33 and 63 dm is assembled by two launches of the projection, at 1, 33 and 63 a k-pair of lora_norm_kernel's B . A is half empty.
    The bars are those of test_norms_and_projection_match_float64 (1e-5 for n, dA, dB, dm; the contractions here are at most 352 long) and of
    test_commit_at_initialisation_is_the_plain_commit_and_merge_equals_commit (1e-5 for the merged master, row by row); every rank index of dA and dB is held to
    1e-5 against the RMS slice norm of the reference, none of which is below a tenth of that RMS (asserted; the smallest is 0.29, a merged row
    whose magnitude drew the factor 0.5).
    Measured on the MI355X, worst over the four ranks: n 4.0e-8, dA 1.5e-7, dB 3.5e-7, dm 3.8e-7, slice 4.4e-7, merged master 1.5e-7, merged row 3.6e-7."""
    _dora_op_case("ragged", arch.ModelConfig("dora-ragged", arch.LLMConfig(layers=1, vocab=512, **RAGGED_LLM), arch.preset("tiny").tower), rank, merge=True)


# ------------------------------------------------------------------------------------------------------------------ 2. commit / merge
def test_commit_at_initialisation_is_the_plain_commit_and_merge_equals_commit():
    model = arch.preset("small")
    B, T = 3, 16
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, 64, B, T)
    tower_out, ids, mask, states, targets = _inputs(model, B, T, 42)
    with torch.no_grad():
        tok = fastvit_hd.projector_forward(w, tower_out.float()).to(DEV)
    rank, alpha = 16, 32.0
    s = alpha / rank
    eng.train_commit(flat)
    pooled0 = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    ws = eng.train_workspace(B, T)
    _, _, g0 = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=torch.zeros_like(flat))
    g0 = g0.clone()
    eng.train_lora_begin(rank, alpha, dora=True)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    lora.init_adapters(lflat, lt, seed=1)              # B = 0
    master0 = flat.clone()
    eng.train_lora_init_magnitude(flat, lflat)         # m = ||W0|| per row
    eng.train_lora_commit(flat, lflat)
    pooled_id = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    _, _, g_id = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=torch.zeros_like(flat))
    torch.cuda.synchronize()
    assert torch.equal(pooled_id, pooled0) and torch.equal(g_id, g0)      # m / n == 1.0f exactly: the operand images (transposed copies included) are the plain commit's
    assert torch.equal(flat, master0)
    named0 = eng.train_named_tensors(master0)
    par = lora.adapter_views(lflat, lt)
    for pre in _targets_of(par):
        e = rel_l2(par[pre + MAG].cpu().reshape(-1), named0[pre + ".weight"].double().cpu().norm(dim=1))
        assert e <= 1e-5, (pre, e)                     # PEFT's initialisation: ||W0|| per row
    # random B, random m != n: adapted commit on the original master == merge into a copy + plain commit
    _random_adapters(eng, lflat, lt, seed=2)
    _random_magnitudes(eng, flat, lflat, lt, seed=3)
    eng.train_lora_commit(flat, lflat)
    pooled_dora = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    _, _, g_dora = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=torch.zeros_like(flat))
    lg = torch.zeros(ltotal, device=DEV)
    eng.train_lora_project(g_dora, lflat, lg)
    torch.cuda.synchronize()
    assert torch.equal(flat, master0)                  # init_magnitude, commit and project never write W0
    assert float((pooled_dora - pooled0).abs().max()) > 0
    merged = flat.clone()
    eng.train_lora_merge(merged, lflat)
    eng.train_commit(merged)
    pooled_merged = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    _, _, g_merged = eng.train_forward_backward(merged, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=torch.zeros_like(flat))
    torch.cuda.synchronize()
    assert torch.equal(pooled_merged, pooled_dora)
    assert torch.equal(g_merged, g_dora)
    named1 = eng.train_named_tensors(merged)
    adapted, worst = set(), 0.0
    for pre in _targets_of(par):
        k = pre + ".weight"
        adapted.add(k)
        V = named0[k].double().cpu() + s * (par[pre + ".lora_B.weight"].double().cpu() @ par[pre + ".lora_A.weight"].double().cpu())
        ref = (par[pre + MAG].double().cpu().reshape(-1) / V.norm(dim=1))[:, None] * V
        e = rel_l2(named1[k].cpu(), ref)
        worst = max(worst, e)
        assert e <= 1e-5, (k, e)
        rows = float(((named1[k].double().cpu() - ref).norm(dim=1) / ref.norm(dim=1)).max())
        assert rows <= 1e-5, (k, rows)                 # ... row by row
    print(f"[dora merge] worst merged matrix rel_l2 {worst:.2e}")
    assert len(adapted) == 7 * model.llm.layers
    for k in named0:
        if k not in adapted:
            assert torch.equal(named0[k], named1[k]), k
    # what merge_lora() does next: B = 0, m <- the merged master's row norms; the adapted commit of the merged master is then the plain one
    for name, v in par.items():
        if name.endswith(".lora_B.weight"):
            v.zero_()
    eng.train_lora_init_magnitude(merged, lflat)
    merged0 = merged.clone()
    eng.train_lora_commit(merged, lflat)
    pooled_again = eng.llm_pooled(ids, mask.sum(1), tok).clone()
    torch.cuda.synchronize()
    assert torch.equal(pooled_again, pooled_dora) and torch.equal(merged, merged0)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. one step against autograd
def _dora_oracle(w, hp, par, s, tower_out, ids, mask, states, targets, lc):
    """autograd over projector -> spliced decoder -> head -> MSE with W' = R(diag(m / n.detach()) (W0 + s B A)) on every adapted matrix (plain LoRA where the
    adapter has no magnitude); R = round to bf16 with a straight-through gradient, the commit's rounding; leaves: A, B, m, head, projector"""
    leaves = {k: v.detach().clone().float().cpu().requires_grad_(True) for k, v in par.items()}
    q = dict(w)
    for k in w:
        if k.startswith("model.mm_projector."):
            leaves[k] = w[k].detach().clone().float().requires_grad_(True)
            q[k] = leaves[k]
    for pre in _targets_of(par):
        V = w[pre + ".weight"].float() + s * (leaves[pre + ".lora_B.weight"] @ leaves[pre + ".lora_A.weight"])
        if pre + MAG in leaves:
            n = V.detach().double().norm(dim=1).float()
            V = (leaves[pre + MAG].reshape(-1) / n)[:, None] * V
        q[pre + ".weight"] = fastvit_hd._r(V)
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


def _check_adamw(eng, lflat, lt, grads, ref):
    """the first clip + AdamW step over exactly the trainable tensors, as test_lora_step_matches_autograd checks it"""
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
        big = (ref["grads"][k].reshape(du.shape) * coef).abs() > 1e-6
        # |first Adam update| <= lr, decoupled weight decay lr . wd . |p|; the difference of two stored fp32 parameters carries the spacing of fp32 at |p|
        pmax = float(p0.abs().max())
        assert float(du.abs().max()) <= 1e-3 + 1e-2 * 1e-3 * pmax + 2.0 ** -22 * max(pmax, 1e-3), k
        if big.any():
            bad = float(((du - dr).abs()[big] > 0.05 * 1e-3 + 1e-2 * dr.abs()[big]).float().mean())
            assert bad <= 5e-3, (k, bad)


def _step_case(name, llm, B, T, hd, rank, targets, dora, rslora, direct=False):
    model = arch.preset("small") if llm is None else arch.ModelConfig(name, llm, arch.preset("tiny").tower)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, hd, B, T)
    tower_out, ids, mask, states, targets_ = _inputs(model, B, T, 42)
    alpha = 2.0 * rank
    cfg = lora.check_config(rank, alpha, targets, dora=dora, rslora=rslora)
    s = lora.scale_of(cfg)
    assert s == (alpha / math.sqrt(rank) if rslora else alpha / rank)
    eng.train_lora_begin(rank, alpha, targets, dora=dora, rslora=rslora)
    lt, ltotal = eng.train_lora_layout()
    want = lora.parse_targets(targets)
    adapters = [t["name"] for t in lt if ".lora_" in t["name"]]
    assert len(adapters) == (3 if dora else 2) * len(want) * model.llm.layers
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    if dora:
        _random_magnitudes(eng, flat, lflat, lt, seed=10)
    master0 = flat.clone()
    eng.train_lora_commit(flat, lflat)
    ws = eng.train_workspace(B, T)
    full_g = None if direct else torch.zeros_like(flat)
    lg = torch.zeros(ltotal, device=DEV)

    def run():
        if direct:
            act, loss, _ = eng.train_lora_forward_backward(flat, lflat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False, lora_grads=lg)
        else:
            act, loss, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False, flat_grads=full_g)
            eng.train_lora_project(full_g, lflat, lg)
        torch.cuda.synchronize()
        return act.clone(), loss.clone(), lg.clone()

    act, loss, grads = run()
    assert torch.equal(flat, master0)
    par = {k: v.clone() for k, v in lora.adapter_views(lflat, lt).items()}
    ref = _dora_oracle(w, hp, par, s, tower_out, ids, mask, states, targets_, lc)
    ra, rl = rel_l2(act.cpu(), ref["pred"]), abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    got = _trainable_named(grads / eng.train_loss_scale(), lt)
    assert set(got) == set(ref["grads"]), sorted(set(got) ^ set(ref["grads"]))[:8]       # the tensors with a gradient are exactly the oracle's leaves
    errs = sorted(((rel_l2(v.cpu(), ref["grads"][k].reshape(v.shape)), k) for k, v in got.items() if float(ref["grads"][k].norm()) > 1e-12), reverse=True)
    tag = ("dora" if dora else "lora") + ("+rslora" if rslora else "") + (" direct" if direct else "")
    print(f"[{tag} {name} r={rank} targets={','.join(want)}] actions rel_l2={ra:.2e} loss rel={rl:.2e}; worst gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:4])
          + f" ({len(errs)} tensors)")
    if dora:
        em = [(e, k) for e, k in errs if k.endswith(MAG)]
        assert len(em) == len(want) * model.llm.layers
        print(f"[{tag} {name} r={rank}] worst magnitude gradient: {em[0][1]} {em[0][0]:.2e}")
    act2, loss2, grads2 = run()
    assert torch.equal(act2, act) and torch.equal(loss2, loss) and torch.equal(grads2, grads)    # bit-identical repeat
    assert ra <= 1e-3 and rl <= 1e-3
    for e, k in errs:
        assert e <= GRAD_TOL, f"gradient of {k}: rel_l2 {e:.3e} > {GRAD_TOL}"
    used = torch.zeros(ltotal, dtype=torch.bool, device=DEV)
    for t in lt:
        used[t["offset"]: t["offset"] + t["numel"]] = True
    _check_adamw(eng, lflat, lt, torch.where(used, grads, torch.zeros_like(grads)), ref)
    eng.close()


@pytest.mark.parametrize("name,llm,B,T,hd,rank,targets", [
    ("small", None, 3, 16, 64, 16, None),
    ("small", None, 3, 16, 64, 4, ("q_proj", "v_proj")),
    ("0.5b-width-4-layers", arch.LLMConfig(hidden=896, layers=4, heads=14, kv_heads=2, head_dim=64, inter=4864, vocab=8192), 4, 32, 128, 16, None),
    ("7b-width-2-layers", arch.LLMConfig(hidden=3584, layers=2, heads=28, kv_heads=4, head_dim=128, inter=18944, vocab=4096), 2, 16, 128, 16, None),
    # two ragged layers at rank 33: the magnitude's gradient assembled by two projection launches on partial strips; control: the unfrozen step's ragged case
    ("ragged-2-layers", arch.LLMConfig(layers=2, vocab=512, **RAGGED_LLM), 3, 16, 64, 33, None),
])
def test_dora_step_matches_autograd(name, llm, B, T, hd, rank, targets):
    """The four cases and the bars of test_lora_step_matches_autograd: actions and loss <= 1e-3, every gradient <= GRAD_TOL (2e-3), lora_magnitude_vector included;
    clip + AdamW over exactly the trainable tensors; bit-identical repeat."""
    _step_case(name, llm, B, T, hd, rank, targets, dora=True, rslora=False)


@pytest.mark.parametrize("direct", [False, True])
def test_rslora_step_matches_autograd(direct):
    """rsLoRA without DoRA: the same oracle with s = alpha / sqrt(r), in the projected and in the direct backward"""
    _step_case("small", None, 3, 16, 64, 16, None, dora=False, rslora=True, direct=direct)


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_engine_usable():
    model = arch.preset("small")
    B, T = 2, 16
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, 64, B, T)
    tower_out, ids, mask, states, targets = _inputs(model, B, T, 42)
    with pytest.raises(FastVLAHipError):
        _lib.check(eng.lib.fv_train_lora_begin_ex(eng.h, 8, 8.0, 127, 4), "fv_train_lora_begin_ex", eng.h)      # an unknown flag
    eng.train_lora_begin(8, 8.0)
    lt, ltotal = eng.train_lora_layout()
    assert not any(t["name"].endswith(MAG) for t in lt)
    lflat = torch.zeros(ltotal, device=DEV)
    with pytest.raises(FastVLAHipError):
        eng.train_lora_init_magnitude(flat, lflat)     # plain LoRA has no magnitudes
    for kw in ({"dora": True}, {"rslora": True}, {"dora": True, "rslora": True}):
        with pytest.raises(FastVLAHipError):
            eng.train_lora_begin(8, 8.0, **kw)         # begun with other flags: as with another rank
    eng.train_lora_begin(8, 8.0)                       # the same arguments again: a no-op
    eng.close()
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, 64, B, T)
    eng.train_lora_begin(8, 8.0, dora=True)
    with pytest.raises(FastVLAHipError):
        eng.train_lora_begin(8, 8.0)
    eng.train_lora_begin(8, 8.0, dora=True)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    eng.train_lora_init_magnitude(flat, lflat)
    eng.train_lora_commit(flat, lflat)
    ws = eng.train_workspace(B, T)
    lg = torch.zeros(ltotal, device=DEV)
    with pytest.raises(FastVLAHipError) as e:
        eng.train_lora_forward_backward(flat, lflat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, lora_grads=lg)
    assert "DoRA" in str(e.value)
    assert float(lg.abs().max()) == 0.0                # refused before anything was enqueued
    full_g = torch.zeros_like(flat)
    eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=full_g)
    eng.train_lora_project(full_g, lflat, lg)          # ... and the projected step still runs
    torch.cuda.synchronize()
    assert torch.isfinite(lg).all() and float(lg.abs().max()) > 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. policy level
def test_policy_level_dora_training_overfits_one_batch_and_round_trips(tmp_path):
    """enable_backbone_training(lora_rank=16, lora_dora=True) + fused_train_step on the fixed batch of the LoRA policy test (its learning rate and criterion)."""
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
        pol.enable_backbone_training(lora_rank=16, lora_dora=True, lora_direct=True)
    st = pol.enable_backbone_training(lora_rank=16, lora_dora=True)
    assert st.lora == {"rank": 16, "alpha": 16.0, "targets": list(lora.TARGETS), "dora": True} and st.lora_direct is False and st.g is not None
    with pytest.raises(RuntimeError):
        pol.enable_backbone_training(lora_rank=16)                                   # running as DoRA: plain LoRA is another configuration
    master0 = st.flat.clone()
    a0 = {k: v.clone() for k, v in lora.adapter_views(st.lflat, st.lora_tensors).items()}
    mags = [k for k in a0 if k.endswith(MAG)]
    assert len(mags) == 7 * pol.model.backbone.engine().model.llm.layers and all(float(a0[k].min()) > 0 for k in mags)
    losses = []
    for i in range(16):
        out = pol.fused_train_step(batch, lr=2e-3, weight_decay=0.0)
        losses.append(float(out["loss"]))
    torch.cuda.synchronize()
    print("[dora policy] loss over 16 steps on one batch:", " ".join(f"{x:.4f}" for x in losses))
    assert all(map(math.isfinite, losses)) and losses[-1] < 0.6 * losses[0]
    assert torch.equal(st.flat[st.front:], master0[st.front:])                  # the decoder master did not move
    a1 = lora.adapter_views(st.lflat, st.lora_tensors)
    assert all(not torch.equal(a0[k], a1[k]) for k in a0)                        # every adapter and every magnitude trained
    pol.eval()
    with torch.no_grad():
        a = pol(batch["images"], batch["states"], batch["tasks"]).clone()
    out_dir = save_policy_checkpoint(pol, tmp_path / "dora")
    ex = json.loads((out_dir / "hip_extras.json").read_text())
    assert ex["lora"] == {"rank": 16, "alpha": 16.0, "targets": list(lora.TARGETS), "dora": True, "file": LORA_FILE}
    ad = torch.load(out_dir / LORA_FILE, map_location="cpu")
    assert ad["config"] == st.lora and "model.layers.0.mlp.down_proj" + MAG in ad["tensors"]
    again = load_policy_from_checkpoint(str(out_dir)).to(DEV)
    assert again._unfrozen.lora == st.lora
    with torch.no_grad():
        a2 = again(batch["images"], batch["states"], batch["tasks"])
    torch.cuda.synchronize()
    assert torch.equal(a2, a)                                                    # a fresh policy computes the very same actions
    # a DoRA file into a plain LoRA run, and the other way round
    plain = FastVLAPolicy(cfg).to(DEV)
    sp = plain.enable_backbone_training(lora_rank=16)
    with pytest.raises(ValueError) as e:
        sp.load_lora_state(ad)
    assert str(ad["config"]) in str(e.value) and str(sp.lora) in str(e.value)
    with pytest.raises(ValueError):
        st.load_lora_state(sp.lora_state())
    # merge_lora(): diag(m / n) (W0 + s B A) into the master, B = 0, m re-initialised; nothing the model computes changes
    pol.merge_lora()
    with torch.no_grad():
        am = pol(batch["images"], batch["states"], batch["tasks"])
    assert torch.equal(am, a)
    assert not torch.equal(st.flat[st.front:], master0[st.front:])
    merged_dir = save_policy_checkpoint(pol, tmp_path / "merged", include_backbone=True)
    assert not (merged_dir / LORA_FILE).exists() and "lora" not in json.loads((merged_dir / "hip_extras.json").read_text())
    fresh = load_policy_from_checkpoint(str(merged_dir)).to(DEV)
    assert fresh._unfrozen is None
    with torch.no_grad():
        a3 = fresh(batch["images"], batch["states"], batch["tasks"])
    torch.cuda.synchronize()
    e = rel_l2(a3.cpu(), a.cpu())
    print(f"[dora policy] merged plain checkpoint vs the adapted policy: actions rel_l2 {e:.2e}")
    assert e <= 1e-5                                                             # (the LoRA policy test's bar for the same comparison)
    for p_ in (pol, again, plain, fresh):
        p_.model.backbone.engine().close()


def test_trainer_fit_in_dora_mode_resumes_bit_for_bit(tmp_path):
    """Trainer.fit() in DoRA mode (the route of test_trainer_fit_in_lora_mode_saves_adapters_and_resumes): the checkpoint records the variant, and a run resumed
    from it on a policy that was never told about LoRA continues bit for bit where the uninterrupted run is."""
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
    lcfg = {"rank": 4, "alpha": 8.0, "targets": ["q_proj", "v_proj", "down_proj"], "dora": True, "rslora": True}

    def fresh(enable=True):
        torch.manual_seed(7)
        p = FastVLAPolicy(cfg).to(DEV)
        if enable:
            p.enable_backbone_training(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"], lora_dora=True, lora_rslora=True)
        return p

    a = fresh()
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=4, **tkw)).fit()
    b = fresh()
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=4, **tkw))
    tb.num_training_steps = 4
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert json.loads((ck / "hip_extras.json").read_text()) == {"splice_image_tokens": True, "train_backbone": True, "train_tower": False, "lora": {**lcfg, "file": LORA_FILE}}
    assert torch.load(ck / LORA_FILE, map_location="cpu")["config"] == lcfg and opt["lora"] == lcfg
    assert opt["m"].numel() == opt["flat"].numel() == b._unfrozen.lflat.numel()
    c = fresh(enable=False)
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=4, resume_from=str(ck), **tkw))
    tc.num_training_steps = 4
    tc.fit()
    torch.cuda.synchronize()
    assert tc.global_step == 4 and c._unfrozen.step_count == 4 and c._unfrozen.lora == lcfg
    assert torch.equal(c._unfrozen.lflat, a._unfrozen.lflat) and torch.equal(c._unfrozen.m, a._unfrozen.m)     # the resumed run IS the uninterrupted one
    assert torch.equal(c._unfrozen.flat, a._unfrozen.flat)
    for p_ in (a, b, c):
        p_.model.backbone.engine().close()


def test_two_rank_dora_step_equals_the_full_batch_step(tmp_path):
    """tools/lora_dp_worker.py --dora once alone and twice as two gloo ranks on the one GPU: the reduced gradient (magnitudes included), its norm and the loss
    reproduce the full-batch step (the bars of test_two_rank_lora_step_equals_the_full_batch_step)."""
    worker = str(ROOT / "tools" / "lora_dp_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    one = tmp_path / "w1"
    one.mkdir()
    r = subprocess.run([sys.executable, worker, "--dora", "--out", str(one)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    two = tmp_path / "w2"
    two.mkdir()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, worker, "--dora", "--out", str(two)], env=dict(env, RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
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
    print(f"[dora dp2 vs full batch] reduced gradient rel_l2 {e:.2e}; grad norm {r0['grad_norm']:.4f} vs {full['grad_norm']:.4f}; payload {r0['payload']} of {r0['full']} floats")
    assert e <= 2e-3 and abs(r0["grad_norm"] - full["grad_norm"]) <= 2e-3 * full["grad_norm"]
    assert abs(0.5 * (r0["loss"] + r1["loss"]) - full["loss"]) <= 1e-4 * abs(full["loss"])
