"""-m gpu: the DIRECT LoRA backward (fv_train_lora_forward_backward in include/fastvla_hip.h; csrc/lora_direct_kernels.hip, csrc/lora_path.inc,
csrc/train_path.inc).

In this mode dA = s (dY B)^T X and dB = s dY^T (X A^T) come straight from the gradient's fp16 rows and the kept activations: the full weight gradient dW' is
never formed and the full-size gradient buffer does not exist.  The projected mode (tests/test_gpu_lora.py) is the yardstick it is held against.
  1. the kernels alone, on random operands in the forms the backward hands them, in all four packed tensors at the 0.5B and 7B layer shapes, against float64;
  2. one whole step against torch.autograd (the oracle, the parameter sets and the bars of test_lora_step_matches_autograd), then the first clip + AdamW step;
  3. UnfrozenState.g is None and the allocator's peak over one step drops by the full gradient buffer;
  4. refusals leave the engine usable;
  5. policy level: overfit, merge, save / load across the two modes, Trainer.fit() + resume, gradient accumulation;
  6. two ranks on the one device reproduce the full-batch step.
"""
import ctypes as C
import gc
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, lib, rel_l2, stream  # noqa: E402
from test_gpu_lora import LLM_05B, LLM_7B, RAGGED_LLM, _lora_oracle, _random_adapters, _slice_stats, _trainable_named  # noqa: E402
from test_gpu_train_unfrozen import GRAD_TOL, _adam_first_update_bound, _inputs, _rig  # noqa: E402
from fastvla_hip import FastVLAHipError, arch, lora  # noqa: E402
from oracle import train_unfrozen  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels alone
def _split_bf16(x):
    """fp32 -> [hi | lo] bf16 columns, as the training forward keeps XN1 / XN2 / ATT; the value the operand holds is hi + lo"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=1).contiguous(), hi.double() + lo.double()


def _direct_operands(kind, part_mask, outs, Np, K, xkind, rank, R, seed):
    """the seeded operands of one fv_op_lora_direct call, on the CPU: dY (fp16 rows), the activation buffer and the float64 value it holds, its row stride and lo
    offset, the parameter buffer, the adapters' offsets per part and the buffer's length"""
    g = torch.Generator().manual_seed(seed)
    dY16 = torch.randn(R, Np, generator=g).to(torch.float16).contiguous()
    x = torch.randn(R, K, generator=g)
    if xkind == 2:
        Xbuf, Xval = _split_bf16(x)
        ldx, lo_off = 2 * K, K
    else:
        Xbuf = x.to(torch.float16).contiguous()
        Xval, ldx, lo_off = Xbuf.double(), K, 0
    a_off, b_off, off = [0, 0, 0], [0, 0, 0], 4           # (a few floats in front: nothing may be written there)
    for p in range(3):
        if outs[p] and part_mask >> p & 1:
            a_off[p] = off
            off += (rank * K + 3) // 4 * 4
            b_off[p] = off
            off += (outs[p] * rank + 3) // 4 * 4
    par = torch.randn(off, generator=g) * 0.3
    return dY16, Xbuf, Xval, ldx, lo_off, par, a_off, b_off, off


def _direct_refs(kind, part_mask, outs, Np, qd, kd, rank, R, s, dY16, Xval, par, a_off, b_off):
    """float64 dA = s (dY B)^T X and dB = s dY^T (X A^T) of every adapter of the call: {part: (dA, dB)}, on the operands' device"""
    dY = dY16.double()                                                       # fp16 read exactly
    K = Xval.shape[1]
    refs = {}
    for p in range(3):
        if not (outs[p] and part_mask >> p & 1):
            continue
        if kind == 1:
            c0 = [0, qd, qd + kd][p]
            dYp = dY[:, c0: c0 + outs[p]]
        elif kind == 2:
            dYp = dY.view(R, Np // 16, 2, 8)[:, :, p, :].reshape(R, Np // 2)
        else:
            dYp = dY
        A = par[a_off[p]: a_off[p] + rank * K].view(rank, K).double()
        B = par[b_off[p]: b_off[p] + outs[p] * rank].view(outs[p], rank).double()
        refs[p] = (s * ((dYp @ B).t() @ Xval), s * (dYp.t() @ (Xval @ A.t())))
    return refs


def _direct_case(tag, kind, part_mask, outs, Np, K, qd, kd, xkind, rank, R, seed, slices=None):
    """one call of fv_op_lora_direct on one packed tensor; outs = logical rows of part 0, 1, 2 (0: the part does not exist).  -> worst rel-L2 of its outputs.
    slices: a dict that receives the worst per-slice error (every rank index of dA, a row, and of dB, a column: _slice_stats) under "err" and the smallest
    reference slice under "floor"."""
    L = lib()
    s = 2.0
    dY16, Xbuf, Xval, ldx, lo_off, par, a_off, b_off, off = _direct_operands(kind, part_mask, outs, Np, K, xkind, rank, R, seed)
    dY16, Xbuf, Xval, par = dY16.to(DEV), Xbuf.to(DEV), Xval.to(DEV), par.to(DEV)
    n = C.c_size_t()
    assert L.fv_op_lora_direct_scratch_floats(R, rank, max(Np, K), C.byref(n)) == 0
    scratch = torch.empty(n.value, device=DEV)

    def run():
        out = torch.full((off,), float("nan"), device=DEV)     # an element the kernels do not write shows
        ao, bo = (C.c_int64 * 3)(*a_off), (C.c_int64 * 3)(*b_off)
        rc = L.fv_op_lora_direct(kind, part_mask, rank, Np, K, qd, kd, ao, bo, dY16.data_ptr(), Xbuf.data_ptr(), xkind, ldx, lo_off, R, par.data_ptr(), out.data_ptr(),
                                 s, scratch.data_ptr(), scratch.numel(), stream())
        assert rc == 0, L.fv_last_error(None)
        torch.cuda.synchronize()
        return out

    out, out2 = run(), run()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))     # fixed summation order: equal bits
    refs = _direct_refs(kind, part_mask, outs, Np, qd, kd, rank, R, s, dY16, Xval, par, a_off, b_off)
    written = torch.zeros(off, dtype=torch.bool, device=DEV)
    worst = 0.0
    for p, (ref_dA, ref_dB) in refs.items():
        got_dA = out[a_off[p]: a_off[p] + rank * K].view(rank, K)
        got_dB = out[b_off[p]: b_off[p] + outs[p] * rank].view(outs[p], rank)
        written[a_off[p]: a_off[p] + rank * K] = True
        written[b_off[p]: b_off[p] + outs[p] * rank] = True
        assert torch.isfinite(got_dA).all() and torch.isfinite(got_dB).all(), (tag, p)
        ea, eb = rel_l2(got_dA, ref_dA), rel_l2(got_dB, ref_dB)
        print(f"[lora direct kernels {tag} r={rank} part {p}] dA rel_l2 {ea:.2e}  dB rel_l2 {eb:.2e}")
        worst = max(worst, ea, eb)
        if slices is not None:
            (sa, fa), (sb, fb) = _slice_stats(got_dA, ref_dA, 1), _slice_stats(got_dB, ref_dB, 0)
            print(f"[lora direct kernels {tag} r={rank} part {p}] worst slice: dA row {sa:.2e}  dB column {sb:.2e}; smallest reference slice / RMS {min(fa, fb):.2f}")
            slices["err"], slices["floor"] = max(slices.get("err", 0.0), sa, sb), min(slices.get("floor", 1e30), fa, fb)
    assert torch.isnan(out[~written]).all(), tag                               # nothing outside the adapters' own ranges is touched
    return worst


@pytest.mark.parametrize("shape", ["0.5b", "7b"])
@pytest.mark.parametrize("rank", [4, 16, 64])
def test_direct_kernels_match_float64_products(shape, rank):
    """rel-L2 <= 2e-5 per output matrix, against float64 products of the values the operands hold (fp16 read exactly, hi + lo of a split value summed).
    Derived, not measured: the kernels round NOTHING to 16 bits -- operands widen to fp32 exactly, A / B are read as fp32, P = dY B and Q = X A^T stay fp32, every
    product is an fp32 fma chain on v_mfma_f32_32x32x2_f32 -- so the only error is fp32 accumulation, about sqrt(K) 2^-24 = 8e-6 at the longest contraction
    here (K = 18944), rounded up to 1e-5 as in test_projection_matches_float64_products; no 2^-11 / sqrt(3) term enters the quadrature sum, and the factor 2
    over it for the tails of one tensor gives 2e-5.  R = 1093 rows: not a multiple of 64, nor of 2."""
    d = LLM_05B if shape == "0.5b" else LLM_7B
    H, I = d["hidden"], d["inter"]
    qd, kd = d["heads"] * d["head_dim"], d["kv_heads"] * d["head_dim"]
    R = 1093
    cases = [("qkv", 1, 7, (qd, kd, kd), qd + 2 * kd, H, 2), ("o", 0, 1, (H, 0, 0), H, qd, 2), ("gate_up", 2, 3, (I, I, 0), 2 * I, H, 2),
             ("down", 0, 1, (H, 0, 0), H, I, 3)]
    if rank == 16:     # a packed tensor only part of which is a target: q and v without k, up without gate
        cases += [("qkv[q,v]", 1, 5, (qd, kd, kd), qd + 2 * kd, H, 2), ("gate_up[up]", 2, 2, (I, I, 0), 2 * I, H, 2)]
    worst = 0.0
    for i, (tag, kind, mask, outs, Np, K, xkind) in enumerate(cases):
        worst = max(worst, _direct_case(f"{shape} {tag}", kind, mask, outs, Np, K, qd, kd, xkind, rank, R, seed=100 * rank + i))
    print(f"[lora direct kernels {shape} r={rank}] worst rel_l2 {worst:.2e}")
    assert worst <= 2e-5, worst


# the ragged layer (RAGGED_LLM in test_gpu_lora.py): q 192, k / v 64 rows, hidden 192, inter 352
RAGGED_QD, RAGGED_KD = RAGGED_LLM["heads"] * RAGGED_LLM["head_dim"], RAGGED_LLM["kv_heads"] * RAGGED_LLM["head_dim"]
# rank -> the tile count NT = ceil(3 r / 32) its three-adapter q|k|v call instantiates, and what else the rank is there for:
#   1   NT 1; odd; 29 padding columns behind three one-column adapters         11  NT 2; adapters end at columns 11, 22, 33: the third straddles tiles 0 | 1
#   24  NT 3; adapters at columns 24 .. 47 and 48 .. 71 straddle tiles 0 | 1, 1 | 2  33  NT 4; odd; every adapter straddles, tile 3 = 3 live + 29 padding columns
#   48  NT 5; every adapter straddles (0 | 1, 1 | 2, 3 | 4)                     63  NT 6; odd; adapters begin at columns 63 and 126, one short of a tile edge
RAGGED_RANKS = [1, 11, 24, 33, 48, 63]
RAGGED_ROWS = 77     # not a multiple of 8: the launcher cuts it into 10 ranges of 8 rows, the last one 5 rows long; three 32-row blocks, the last 13 rows


def _ragged_direct_cases(rank):
    """(tag, kind, part mask, outs, Np, K, xkind, R) of every call test_direct_kernels_at_ragged_shapes makes at this rank"""
    H, I, qd, kd, R = RAGGED_LLM["hidden"], RAGGED_LLM["inter"], RAGGED_QD, RAGGED_KD, RAGGED_ROWS
    cases = [
        ("qkv", 1, 7, (qd, kd, kd), qd + 2 * kd, H, 2, R),            # three adapters: NT as listed above; parts begin at packed columns 192 and 256
        ("o", 0, 1, (H, 0, 0), H, qd, 2, R),                          # one adapter: NT 1 (2 from rank 33 on), padding behind it; 12 chunks over 8 waves
        ("gate_up", 2, 3, (I, I, 0), 2 * I, H, 2, R),                 # two adapters interleaved by 8 columns: every tile of V against every tile of dY
        ("down", 0, 1, (H, 0, 0), H, I, 3, R),                        # fp16 activation rows; K = 352 = 22 chunks over 8 waves: uneven ranges (2 or 3 chunks)
        ("thin", 0, 1, (32, 0, 0), 32, 32, 3, R),                     # 2 chunks over 8 waves: six EMPTY ranges; one wave of four in the outer kernel's block
    ]
    if rank in (11, 24, 48):     # a packed tensor only part of which is a target: the slots are not the parts
        cases += [("qkv[q,v]", 1, 5, (qd, kd, kd), qd + 2 * kd, H, 2, R), ("qkv[k]", 1, 2, (qd, kd, kd), qd + 2 * kd, H, 2, R),
                  ("gate_up[gate]", 2, 1, (I, I, 0), 2 * I, H, 2, R), ("gate_up[up]", 2, 2, (I, I, 0), 2 * I, H, 2, R)]
    if rank == 24:               # one row (one range, one 8-row round with seven rows of zeros) and exactly one 32-row block
        cases += [("qkv R=1", 1, 7, (qd, kd, kd), qd + 2 * kd, H, 2, 1), ("qkv R=32", 1, 7, (qd, kd, kd), qd + 2 * kd, H, 2, 32)]
    return cases


@pytest.mark.parametrize("rank", RAGGED_RANKS)
def test_direct_kernels_at_ragged_shapes(rank):
    """The kernels alone at every rank class and at the ragged layer's shapes (hidden 192, q | k | v 192 | 64 | 64, inter 352), R = 77 rows: what each rank and
    each case is there for stands beside RAGGED_RANKS and in _ragged_direct_cases.  The bar of test_direct_kernels_match_float64_products, 2e-5 per output matrix
    (fp32 accumulation only; derived at K = 18944, the contractions here are at most 704 long), and the same 2e-5 for EVERY SLICE -- each rank index of dA (a row)
    and of dB (a column) -- measured against the RMS slice norm of the reference matrix: a whole-matrix rel-L2 lets one wrong rank index of 63 through.  No
    reference slice is smaller than a tenth of that RMS (asserted; the smallest over all cases with R >= 32 is 0.52), so no slice is judged against a norm it
    does not have.  The one-row case is exempt from that floor, not from the bar: its dA row j is the scalar P_j = dY . B[:, j] times X, a Gaussian draw per
    slice, and 144 of them never all stay above a tenth of their RMS whatever the seed.
    Measured on the MI355X, worst over all cases: per matrix 1.7e-7, per slice 5.9e-7 (rank 24, R = 1)."""
    worst, st = 0.0, {}
    for i, (tag, kind, mask, outs, Np, K, xkind, R) in enumerate(_ragged_direct_cases(rank)):
        one = {}
        worst = max(worst, _direct_case(f"ragged {tag}", kind, mask, outs, Np, K, RAGGED_QD, RAGGED_KD, xkind, rank, R, seed=100 * rank + i, slices=one))
        assert R == 1 or one["floor"] >= 0.1, (tag, one)
        st["err"] = max(st.get("err", 0.0), one["err"])
        if R > 1:
            st["floor"] = min(st.get("floor", 1e30), one["floor"])
    print(f"[lora direct kernels ragged r={rank}] worst rel_l2 {worst:.2e}; worst slice {st['err']:.2e}; smallest reference slice / RMS {st['floor']:.2f}")
    assert worst <= 2e-5, worst
    assert st["err"] <= 2e-5, st


# ------------------------------------------------------------------------------------------------------------------ 2. one step against autograd
@pytest.mark.parametrize("name,llm,B,T,hd,rank,targets", [
    ("small", None, 3, 16, 64, 16, None),
    ("small", None, 3, 16, 64, 4, ("q_proj", "v_proj")),
    ("0.5b-width-4-layers", arch.LLMConfig(hidden=896, layers=4, heads=14, kv_heads=2, head_dim=64, inter=4864, vocab=8192), 4, 32, 128, 16, None),
    ("7b-width-2-layers", arch.LLMConfig(hidden=3584, layers=2, heads=28, kv_heads=4, head_dim=128, inter=18944, vocab=4096), 2, 16, 128, 16, None),
    # two ragged layers at rank 24: q | k | v runs NT = 3, gate / up a straddled NT = 2, o and down a padded NT = 1; control: the unfrozen step's ragged case
    ("ragged-2-layers", arch.LLMConfig(layers=2, vocab=512, **RAGGED_LLM), 3, 16, 64, 24, None),
])
def test_direct_step_matches_autograd(name, llm, B, T, hd, rank, targets):
    """actions and loss <= 1e-3, every trainable tensor's gradient <= GRAD_TOL (the project's 2e-3) against _lora_oracle(rounded=True); the tensors with a
    gradient are exactly the oracle's leaves; bit-identical repeat; the master is not written; then the first clip + AdamW step as test_lora_step_matches_autograd
    checks it.  The distance to the projected mode's gradients of the same step is printed for the record (both are bounded against autograd)."""
    model = arch.preset("small") if llm is None else arch.ModelConfig(name, llm, arch.preset("tiny").tower)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, hd, B, T)
    tower_out, ids, mask, states, targets_ = _inputs(model, B, T, 42)
    alpha = 2.0 * rank
    s = alpha / rank
    eng.train_lora_begin(rank, alpha, targets)
    lt, ltotal = eng.train_lora_layout()
    want = lora.parse_targets(targets)
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    master0 = flat.clone()
    eng.train_lora_commit(flat, lflat)
    ws = eng.train_workspace(B, T)

    def run():
        lg = torch.full((ltotal,), float("nan"), device=DEV)
        act, loss, _ = eng.train_lora_forward_backward(flat, lflat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False, lora_grads=lg)
        torch.cuda.synchronize()
        return act.clone(), loss.clone(), lg

    act, loss, grads = run()
    assert torch.equal(flat, master0)
    used = torch.zeros(ltotal, dtype=torch.bool, device=DEV)
    for t in lt:
        used[t["offset"]: t["offset"] + t["numel"]] = True
    assert torch.isfinite(grads[used]).all()               # every element of every trainable tensor was written
    par = {k: v.clone() for k, v in lora.adapter_views(lflat, lt).items()}
    ref = _lora_oracle(w, hp, par, s, tower_out, ids, mask, states, targets_, lc, rounded=True)
    ra, rl = rel_l2(act.cpu(), ref["pred"]), abs(float(loss) - float(ref["loss"])) / float(ref["loss"])

    def grad_errors(g):
        got = _trainable_named(g / eng.train_loss_scale(), lt)
        assert set(got) == set(ref["grads"]), sorted(set(got) ^ set(ref["grads"]))[:8]
        return sorted(((rel_l2(v.cpu(), ref["grads"][k]), k) for k, v in got.items() if float(ref["grads"][k].norm()) > 1e-12), reverse=True)

    errs = grad_errors(grads)
    print(f"[lora direct {name} r={rank} targets={','.join(want)}] actions rel_l2={ra:.2e} loss rel={rl:.2e}; worst gradients: "
          + "; ".join(f"{k} {e:.2e}" for e, k in errs[:4]) + f" ({len(errs)} tensors)")
    # for the record: the projected mode's gradients of the same step
    full_g, lgp = torch.zeros_like(flat), torch.zeros(ltotal, device=DEV)
    actp, lossp, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False, flat_grads=full_g)
    eng.train_lora_project(full_g, lflat, lgp)
    torch.cuda.synchronize()
    gd, gp = _trainable_named(grads, lt), _trainable_named(lgp, lt)
    dist = max(((rel_l2(gd[k], gp[k]), k) for k in gd if float(gp[k].norm()) > 0), default=(0.0, ""))
    print(f"[lora direct {name} r={rank}] worst distance to the projected mode's gradients: {dist[1]} {dist[0]:.2e}; actions equal: {torch.equal(actp, act)}")
    del full_g
    act2, loss2, grads2 = run()
    assert torch.equal(act2, act) and torch.equal(loss2, loss) and torch.equal(grads2[used], grads[used])    # bit-identical repeat
    assert ra <= 1e-3 and rl <= 1e-3
    for e, k in errs:
        assert e <= GRAD_TOL, f"gradient of {k}: rel_l2 {e:.3e} > {GRAD_TOL}"
    grads = torch.where(used, grads, torch.zeros_like(grads))       # (the padding between tensors is no parameter)
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
        assert float(du.abs().max()) <= _adam_first_update_bound(float(p0.abs().max())), k
        if big.any():
            bad = float(((du - dr).abs()[big] > 0.05 * 1e-3 + 1e-2 * dr.abs()[big]).float().mean())
            assert bad <= 5e-3, (k, bad)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the buffer is gone
def _policy_cfg(model_name="small", seed=41):
    from vla_fastvlm.fastvla import FastVLAConfig
    return FastVLAConfig(vlm_model_name=f"synthetic:{model_name}:{seed}", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)


def _fixed_batch(B=4):
    g = torch.Generator().manual_seed(6)
    return {"images": torch.rand(B, 3, 96, 128, generator=g).to(DEV), "states": torch.randn(B, 14, generator=g).to(DEV),
            "actions": torch.randn(B, 14, generator=g).to(DEV), "tasks": ["pick up the red cube", "open the drawer", "push", "pick up the red cube"][:B]}


@pytest.mark.parametrize("model_name", ["small", "0.5b-width-4-layers"])
def test_the_full_gradient_buffer_is_gone(model_name):
    """UnfrozenState.g is None in direct mode, and the allocator's peak over one step (above what was allocated before the policy existed) is lower than the
    projected mode's for the same shapes by at least 0.9 x 4 x total bytes -- the full-size gradient buffer."""
    from vla_fastvlm.fastvla import FastVLAPolicy
    if model_name != "small":
        arch.PRESETS[model_name] = arch.ModelConfig(model_name, arch.LLMConfig(hidden=896, layers=4, heads=14, kv_heads=2, head_dim=64, inter=4864, vocab=8192),
                                                    arch.preset("small").tower)
    try:
        batch = _fixed_batch(2)
        peaks, total = {}, None
        for direct in (False, True):
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.manual_seed(5)
            pol = FastVLAPolicy(_policy_cfg(model_name)).to(DEV)
            pol.train()
            st = pol.enable_backbone_training(lora_rank=8, lora_direct=direct)
            assert st.lora_direct is direct and (st.g is None) == direct
            total = st.total
            pol.fused_train_step(batch, lr=1e-3)           # (the workspace and every lazily made buffer exist after this one)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            pol.fused_train_step(batch, lr=1e-3)
            torch.cuda.synchronize()
            peaks[direct] = torch.cuda.max_memory_allocated() - base
            pol.model.backbone.engine().close()
            del pol, st
        saved = peaks[False] - peaks[True]
        print(f"[lora direct memory {model_name}] peak over one step: projected {peaks[False] / 2**20:.1f} MiB, direct {peaks[True] / 2**20:.1f} MiB, "
              f"saved {saved / 2**20:.1f} MiB; the full gradient buffer: {4 * total / 2**20:.1f} MiB")
        assert saved >= 0.9 * 4 * total, (peaks, total)
    finally:
        arch.PRESETS.pop("0.5b-width-4-layers", None)


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_engine_usable():
    from fastvla_hip import FastVLAEngine, weights
    model = arch.preset("small")
    B, T = 2, 16
    w, eng, tensors, total, nb, flat, lc, hp = _rig(model, 41, 64, B, T)
    tower_out, ids, mask, states, targets_ = _inputs(model, B, T, 42)
    ws = eng.train_workspace(B, T)
    dummy = torch.zeros(1024, device=DEV)

    def step(lflat):
        return eng.train_lora_forward_backward(flat, lflat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False)

    with pytest.raises(FastVLAHipError) as ei:          # no fv_train_lora_begin
        step(dummy)
    assert ei.value.status == -2 and "fv_train_lora_begin" in str(ei.value)      # FV_ERR_STATE
    eng.train_lora_begin(8, 16.0)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    eng.train_lora_commit(flat, lflat)
    for kw in (dict(grad_split=1), dict(wgrad_f16=False)):           # non-default backward options
        eng.train_set_options(**kw)
        with pytest.raises(FastVLAHipError) as ei:
            step(lflat)
        assert ei.value.status == -5 and "fv_train_set_options" in str(ei.value)      # FV_ERR_UNSUPPORTED
    eng.train_set_options()
    eng.train_lora_commit(flat, lflat)
    eng.train_set_forward_f16(True)                                   # the fp16 training forward is not supported in this mode
    with pytest.raises(FastVLAHipError) as ei:
        step(lflat)
    assert ei.value.status == -5 and "fv_train_set_forward_f16" in str(ei.value)
    eng.train_set_forward_f16(False)
    eng.train_lora_commit(flat, lflat)
    act, loss, lg = step(lflat)                                       # a following valid step runs ...
    actp, lossp, gfull = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False)
    torch.cuda.synchronize()
    assert torch.equal(act, actp) and torch.equal(loss, lossp)        # ... and its forward is the projected mode's
    hv, hvp = eng.head_views(lg[: eng.head_numel()]), eng.head_views(gfull[: eng.head_numel()])
    assert all(torch.equal(hv[k], hvp[k]) for k in hv)                # the head's gradients: the same kernel on the same operands
    eng.close()
    # a trained tower: LoRA (either backward) is refused before a state exists
    eng2 = FastVLAEngine(model, state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng2.load_weights(weights.init_backbone(model, seed=41))
    eng2.train_begin()
    eng2.train_tower_begin()
    with pytest.raises(FastVLAHipError) as ei:
        eng2.train_lora_begin(8, 16.0)
    assert ei.value.status == -5                                      # FV_ERR_UNSUPPORTED: adapters go with a frozen tower ...
    with pytest.raises(FastVLAHipError) as ei:
        eng2.train_lora_forward_backward(flat, lflat, tower_out.to(DEV), ids, mask.sum(1), states, targets_, ws, training=False)
    assert ei.value.status == -2 and "fv_train_lora_begin" in str(ei.value)      # ... so the direct step finds no LoRA state (FV_ERR_STATE)
    eng2.close()
    from vla_fastvlm.fastvla import FastVLAPolicy
    pol = FastVLAPolicy(_policy_cfg())
    with pytest.raises(ValueError):
        pol.enable_backbone_training(lora_direct=True)                # lora_direct without a rank
    with pytest.raises(ValueError):
        pol.enable_backbone_training(tower=True, lora_rank=8, lora_direct=True)
    assert pol._unfrozen is None


# ------------------------------------------------------------------------------------------------------------------ 5. policy level
def test_policy_level_direct_training_overfits_and_round_trips_across_modes(tmp_path):
    """enable_backbone_training(lora_rank=8, lora_direct=True) on the fixed batch, steps, learning rate and criterion of
    test_policy_level_lora_training_overfits_one_batch_and_round_trips; checkpoints written in one mode load in the other."""
    from vla_fastvlm.fastvla import FastVLAPolicy
    from vla_fastvlm.utils import load_policy_from_checkpoint, save_policy_checkpoint
    from vla_fastvlm.utils.checkpoint import LORA_FILE, load_lora_adapters, read_extras
    torch.manual_seed(5)
    cfg = _policy_cfg()
    batch = _fixed_batch(4)
    pol = FastVLAPolicy(cfg).to(DEV)
    pol.train()
    st = pol.enable_backbone_training(lora_rank=8, lora_direct=True)
    assert st.lora == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS)} and st.lora_direct is True and st.g is None    # the flag is no part of the adapter config
    master0 = st.flat.clone()
    a0 = {k: v.clone() for k, v in lora.adapter_views(st.lflat, st.lora_tensors).items()}
    losses = []
    for i in range(16):
        out = pol.fused_train_step(batch, lr=2e-3, weight_decay=0.0)
        losses.append(float(out["loss"]))
    torch.cuda.synchronize()
    print("[lora direct policy] loss over 16 steps on one batch:", " ".join(f"{x:.4f}" for x in losses))
    assert all(map(math.isfinite, losses)) and losses[-1] < 0.6 * losses[0]
    assert torch.equal(st.flat[st.front:], master0[st.front:])                  # the decoder master did not move
    assert torch.equal(st.flat[: st.front], st.lflat[: st.front])
    a1 = lora.adapter_views(st.lflat, st.lora_tensors)
    assert all(not torch.equal(a0[k], a1[k]) for k in a0)                        # every adapter trained
    pol.eval()
    with torch.no_grad():
        a = pol(batch["images"], batch["states"], batch["tasks"]).clone()

    def load_into(p_, d):
        """what load_policy_from_checkpoint does with the files, on a policy that is already in LoRA mode"""
        sd = torch.load(d / "policy_state_dict.pt", map_location="cpu")
        p_.load_state_dict({k: sd[k] for k in p_.state_dict() if k in sd}, strict=False)
        load_lora_adapters(p_, d, read_extras(d)["lora"])
        p_.eval()
        with torch.no_grad():
            r = p_(batch["images"], batch["states"], batch["tasks"]).clone()
        torch.cuda.synchronize()
        return r

    # saved in direct mode ...
    d_dir = save_policy_checkpoint(pol, tmp_path / "direct")
    ex = json.loads((d_dir / "hip_extras.json").read_text())
    assert ex["lora"] == {"rank": 8, "alpha": 8.0, "targets": list(lora.TARGETS), "file": LORA_FILE, "direct": True}
    assert torch.load(d_dir / LORA_FILE, map_location="cpu")["config"] == st.lora           # the adapter file's config is mode-free
    fresh = load_policy_from_checkpoint(str(d_dir)).to(DEV)                                   # ... a fresh policy comes up in the recorded mode
    assert fresh._unfrozen.lora_direct is True and fresh._unfrozen.g is None
    with torch.no_grad():
        af = fresh(batch["images"], batch["states"], batch["tasks"])
    assert torch.equal(af, a)
    proj = FastVLAPolicy(cfg).to(DEV)                                                         # ... a policy started in projected mode keeps its mode
    sp = proj.enable_backbone_training(lora_rank=8)
    assert sp.lora_direct is False and sp.g is not None
    with pytest.raises(RuntimeError):
        proj.enable_backbone_training(lora_rank=8, lora_direct=True)                          # a running state is not switched, and says so
    assert torch.equal(load_into(proj, d_dir), a) and proj._unfrozen is sp and sp.lora_direct is False
    # the reverse: trained and saved in projected mode, loaded into a policy started in direct mode
    proj.train()
    for i in range(2):
        proj.fused_train_step(batch, lr=2e-3, weight_decay=0.0)
    proj.eval()
    with torch.no_grad():
        ap = proj(batch["images"], batch["states"], batch["tasks"]).clone()
    p_dir = save_policy_checkpoint(proj, tmp_path / "projected")
    assert "direct" not in json.loads((p_dir / "hip_extras.json").read_text())["lora"]       # a missing key means projected
    fresh_p = load_policy_from_checkpoint(str(p_dir)).to(DEV)
    assert fresh_p._unfrozen.lora_direct is False
    dpol = FastVLAPolicy(cfg).to(DEV)
    sd_ = dpol.enable_backbone_training(lora_rank=8, lora_direct=True)
    assert torch.equal(load_into(dpol, p_dir), ap) and sd_.lora_direct is True and sd_.g is None
    # gradient accumulation over two micro-batches == the full-batch step, in direct mode
    pa, pb = FastVLAPolicy(cfg).to(DEV), FastVLAPolicy(cfg).to(DEV)
    for p_ in (pa, pb):
        p_.train()
    sa, sb = pa.enable_backbone_training(lora_rank=8, lora_direct=True), pb.enable_backbone_training(lora_rank=8, lora_direct=True)
    for s_ in (sa, sb):
        s_.lflat.copy_(st.lflat)
        s_.commit()
    pa.fused_train_step(batch, lr=1e-3)
    half = lambda lo, hi: {k: v[lo:hi] for k, v in batch.items()}   # noqa: E731
    pb.fused_train_step(half(0, 2), lr=1e-3, grad_accum_steps=2)
    pb.fused_train_step(half(2, 4), lr=1e-3, grad_accum_steps=2)
    torch.cuda.synchronize()
    e = rel_l2((sb.acc / 2).cpu(), sa.lg.cpu())
    print(f"[lora direct policy] two accumulated half batches vs the full batch: rel_l2 {e:.2e}")
    assert sb.acc.numel() == sb.lflat.numel() and e <= GRAD_TOL
    # merge_lora(), then a plain backbone export reproduces the actions
    pol.merge_lora()
    with torch.no_grad():
        am = pol(batch["images"], batch["states"], batch["tasks"])
    assert torch.equal(am, a)
    merged_dir = save_policy_checkpoint(pol, tmp_path / "merged", include_backbone=True)
    assert not (merged_dir / LORA_FILE).exists() and "lora" not in json.loads((merged_dir / "hip_extras.json").read_text())
    plain = load_policy_from_checkpoint(str(merged_dir)).to(DEV)
    assert plain._unfrozen is None
    with torch.no_grad():
        a3 = plain(batch["images"], batch["states"], batch["tasks"])
    torch.cuda.synchronize()
    e = rel_l2(a3.cpu(), a.cpu())
    print(f"[lora direct policy] merged plain checkpoint vs the adapted policy: actions rel_l2 {e:.2e}")
    assert e <= 1e-5
    for p_ in (pol, fresh, proj, fresh_p, dpol, pa, pb, plain):
        p_.model.backbone.engine().close()


def test_trainer_fit_in_direct_mode_resumes_bit_for_bit(tmp_path):
    """Trainer.fit() in direct LoRA mode, and a run resumed from its checkpoint on a policy that was never told about LoRA: it comes up in direct mode (the
    checkpoint records it) and continues bit for bit where the uninterrupted run is (the route of test_trainer_fit_in_lora_mode_saves_adapters_and_resumes)."""
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
            p.enable_backbone_training(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"], lora_direct=True)
        return p

    a = fresh()
    master0 = a._unfrozen.flat.clone()
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=4, **tkw)).fit()
    b = fresh()
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=4, **tkw))
    tb.num_training_steps = 4
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert json.loads((ck / "hip_extras.json").read_text())["lora"] == {**lcfg, "file": LORA_FILE, "direct": True}
    assert opt["lora"] == lcfg and torch.load(ck / LORA_FILE, map_location="cpu")["config"] == lcfg      # neither file carries the run's mode
    c = fresh(enable=False)
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=4, resume_from=str(ck), **tkw))
    tc.num_training_steps = 4
    tc.fit()
    torch.cuda.synchronize()
    assert tc.global_step == 4 and c._unfrozen.step_count == 4 and c._unfrozen.lora == lcfg
    assert c._unfrozen.lora_direct is True and c._unfrozen.g is None
    assert torch.equal(c._unfrozen.lflat, a._unfrozen.lflat) and torch.equal(c._unfrozen.m, a._unfrozen.m)
    front = a._unfrozen.front
    assert torch.equal(a._unfrozen.flat[front:], master0[front:]) and torch.equal(c._unfrozen.flat, a._unfrozen.flat)
    for p_ in (a, b, c):
        p_.model.backbone.engine().close()


# ------------------------------------------------------------------------------------------------------------------ 6. two ranks
def test_two_rank_direct_step_equals_the_full_batch_step(tmp_path):
    """tools/lora_dp_worker.py --direct, once alone and as two gloo ranks on the one GPU: the bar of test_two_rank_lora_step_equals_the_full_batch_step."""
    worker = str(ROOT / "tools" / "lora_dp_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    one = tmp_path / "w1"
    one.mkdir()
    r = subprocess.run([sys.executable, worker, "--out", str(one), "--direct"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    two = tmp_path / "w2"
    two.mkdir()
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, worker, "--out", str(two), "--direct"], env=dict(env, RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
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
    print(f"[lora direct dp2 vs full batch] reduced gradient rel_l2 {e:.2e}; grad norm {r0['grad_norm']:.4f} vs {full['grad_norm']:.4f}")
    assert e <= 2e-3 and abs(r0["grad_norm"] - full["grad_norm"]) <= 2e-3 * full["grad_norm"]
    assert abs(0.5 * (r0["loss"] + r1["loss"]) - full["loss"]) <= 1e-4 * abs(full["loss"])
