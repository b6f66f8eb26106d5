"""-m gpu: per-dimension / per-step weights of the chunked action loss (fv_head_set_loss_weights) and the per-dimension error (fv_head_loss_per_dim) -- the
weighted kernel instance against float64, its bit rules (all-ones weights, zero weights over poisoned targets, two runs), the setters, the head step
against autograd, and through the policy on every training route.

Bars: those of test_gpu_action_chunk.py -- loss and metrics relative 1e-5; dL/dactions per element |d| <= 2e-5 max(1e-3 max|ref|, |ref|); head gradients
2e-5 max(1e-3, max|ref|) per tensor; the per-dimension error relative 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chunk_loss_util import KINDS, chunk_loss_ref, ragged_pad  # noqa: E402
from gpu_util import DEV, call, lib, stream  # noqa: E402
from fastvla_hip import HEAD_KEYS, _lib  # noqa: E402
from oracle import head  # noqa: E402
from test_gpu_action_chunk import BETA, KIND_ID, _chunk_batch, _dev, _flat, _head_engine, _head_io, _head_params, _loss_inputs, _masks, _op_loss  # noqa: E402
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy  # noqa: E402


def weighted_loss_ref(a, t, pad, dim_w, step_w, kind="mse", beta=1.0, loss_scale=1.0):
    """float64: om = dim_w[a] step_w[k]; loss = sum_valid om rho(d) / n, g = loss_scale om rho'(d) / n, n = ALL elements.  An element with om == 0 is
    selected away like a padded one (its target never enters the arithmetic).  mse (unweighted) = sum over the selected elements of d^2 / n; valid counts
    pads only."""
    a, t = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B, K, A = a.shape
    n = a.size
    om = np.asarray(step_w, dtype=np.float64).reshape(1, K, 1) * np.asarray(dim_w, dtype=np.float64).reshape(1, 1, A)
    w = np.ones((B, K), dtype=bool) if pad is None else ~np.asarray(pad, dtype=bool).reshape(B, K)
    sel = np.broadcast_to(w[:, :, None], a.shape) & np.broadcast_to(om != 0, a.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(sel, a - np.where(sel, t, 0.0), 0.0)
    ad = np.abs(d)
    if kind == "mse":
        rho, drho = d * d, 2.0 * d
    elif kind == "l1":
        rho, drho = ad, np.sign(d)
    else:
        rho, drho = np.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta), np.where(ad < beta, d / beta, np.sign(d))
    rho, drho = np.where(sel, om * rho, 0.0), np.where(sel, om * drho, 0.0)
    return {"loss": float(rho.sum() / n), "mse": float(np.where(sel, d * d, 0.0).sum() / n), "valid": float(w.sum() / (B * K)), "g": loss_scale * drho / n}


def _weights(A, K, seed):
    """fp32 weights, uniform in [0, 4], at least one exact 0 per vector"""
    g = torch.Generator().manual_seed(seed)
    dim_w, step_w = torch.rand(A, generator=g) * 4.0, torch.rand(K, generator=g) * 4.0
    dim_w[int(torch.randint(0, A, (1,), generator=g))] = 0.0
    step_w[int(torch.randint(0, K, (1,), generator=g))] = 0.0
    return dim_w, step_w


def _op_weighted(a, t, pad, dim_w, step_w, kind, beta=BETA, loss_scale=1.0):
    """chunk_loss_kernel<WEIGHTED> + fold alone (fv_op_chunk_loss_weighted) -> loss, metrics (2,), g (B, K, A) on the CPU"""
    B, K, A = a.shape
    ad, td = a.to(DEV).contiguous(), t.to(DEV).contiguous()
    pd = None if pad is None else torch.as_tensor(pad).to(DEV, torch.uint8).contiguous()
    dw, sw = dim_w.to(DEV, torch.float32).contiguous(), step_w.to(DEV, torch.float32).contiguous()
    g = torch.full((B, K, A), float("nan"), device=DEV)
    part, out = torch.full((768,), float("nan"), device=DEV), torch.full((3,), float("nan"), device=DEV)
    call(lib().fv_op_chunk_loss_weighted(ad.data_ptr(), td.data_ptr(), None if pd is None else pd.data_ptr(), dw.data_ptr(), sw.data_ptr(), g.data_ptr(),
                                         part.data_ptr(), part.numel(), out.data_ptr(), out[1:].data_ptr(), a.numel(), A, K, KIND_ID[kind], beta, loss_scale,
                                         stream()), "fv_op_chunk_loss_weighted")
    torch.cuda.synchronize()
    return float(out[0]), out[1:].cpu(), g.cpu()


def _check(got, ref, where):
    loss, met, g = got
    assert np.isfinite(loss) and torch.isfinite(met).all() and torch.isfinite(g).all(), (where, "non-finite")
    worst = {}
    for what, have, want in (("loss", loss, ref["loss"]), ("mse", float(met[0]), ref["mse"]), ("valid", float(met[1]), ref["valid"])):
        err = abs(have - want) / abs(want) if want else abs(have)
        worst[what] = err / 1e-5
        assert err <= 1e-5, (where, what, have, want)
    rg = torch.from_numpy(ref["g"])
    bar = 2e-5 * torch.maximum(1e-3 * rg.abs().max(), rg.abs())
    diff = (g.double() - rg).abs()
    worst["g"] = float((diff / bar).max()) if float(rg.abs().max()) > 0 else 0.0
    assert bool((diff <= bar).all()), (where, "g", float((diff / bar.clamp_min(1e-300)).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ 1. the weighted instance against float64
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 5), (2, 7, 3), (9, 7, 14), (64, 50, 14)])
def test_weighted_loss_kernel_matches_float64(shape, kind):
    B, K, A = shape
    a, t0 = _loss_inputs(B, K, A, seed=B * 100 + K)
    dim_w, step_w = _weights(A, K, seed=B + K)
    assert bool((dim_w == 0).any()) and bool((step_w == 0).any())
    zero = ((step_w.view(1, K, 1) * dim_w.view(1, 1, A)) == 0).expand(B, K, A)
    worst = {}
    for ls in (1.0, 4096.0):
        for name, (pad, t) in _masks(B, K, t0).items():
            got = _op_weighted(a, t, pad, dim_w, step_w, kind, loss_scale=ls)
            ref = weighted_loss_ref(a.numpy(), t.numpy(), pad, dim_w.numpy(), step_w.numpy(), kind, BETA, loss_scale=ls)
            for k, v in _check(got, ref, (name, ls)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert bool((got[2][zero] == 0).all()), name                      # a zero weight gives exactly 0
            if pad is not None:
                assert bool((got[2][torch.from_numpy(pad)] == 0).all()), name
            if name == "all-padded":
                assert got[0] == 0.0 and float(got[1][0]) == 0.0 and float(got[1][1]) == 0.0 and bool((got[2] == 0).all())
    pad, t = _masks(B, K, t0)["ragged"]
    r1, r2 = _op_weighted(a, t, pad, dim_w, step_w, kind), _op_weighted(a, t, pad, dim_w, step_w, kind)
    assert r1[0] == r2[0] and torch.equal(r1[1], r2[1]) and torch.equal(r1[2], r2[2])      # two runs agree bit for bit
    print(f"[weighted chunk loss {kind} {shape}] worst error / bar: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(3, 4, 5), (9, 7, 14), (64, 50, 14)])
def test_all_ones_weights_are_the_unweighted_kernel_bit_for_bit(shape, kind):
    B, K, A = shape
    a, t0 = _loss_inputs(B, K, A, seed=B * 100 + K)
    for ls in (1.0, 4096.0):
        for name, (pad, t) in _masks(B, K, t0).items():
            plain = _op_loss(a, t, pad, kind, loss_scale=ls)
            ones = _op_weighted(a, t, pad, torch.ones(A), torch.ones(K), kind, loss_scale=ls)
            assert plain[0] == ones[0] and torch.equal(plain[1], ones[1]) and torch.equal(plain[2], ones[2]), (name, ls)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_weights_select_poisoned_targets_away(kind):
    B, K, A = 9, 7, 14
    a, t = _loss_inputs(B, K, A, seed=5)
    dim_w, step_w = torch.ones(A) * 2.0, torch.ones(K) * 0.5
    dim_w[A - 1] = 0.0                                                        # the gripper channel, say
    step_w[K - 2] = 0.0
    vals = torch.tensor([float("nan"), float("inf"), float("-inf")])
    bad = t.clone()
    bad[:, :, A - 1] = vals[torch.arange(B * K) % 3].view(B, K)
    bad[:, K - 2, :] = vals[torch.arange(B * A) % 3].view(B, A)
    for pad in (None, ragged_pad(B, K, seed=1)):
        clean, got = _op_weighted(a, t, pad, dim_w, step_w, kind), _op_weighted(a, bad, pad, dim_w, step_w, kind)
        assert np.isfinite(got[0]) and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
        assert bool((got[2][:, :, A - 1] == 0).all()) and bool((got[2][:, K - 2, :] == 0).all())
        # what a zero-weight element's target holds changes no bit of anything
        assert got[0] == clean[0] and torch.equal(got[1], clean[1]) and torch.equal(got[2], clean[2])
        _check(got, weighted_loss_ref(a.numpy(), bad.numpy(), pad, dim_w.numpy(), step_w.numpy(), kind, BETA), "poisoned")


def test_weighted_kernel_unaligned_pointers_take_the_scalar_form():
    B, K, A = 5, 3, 7
    a, t = _loss_inputs(B, K, A, seed=11)
    pad = ragged_pad(B, K, seed=2)
    dim_w, step_w = _weights(A, K, seed=4)
    n = a.numel()
    buf = torch.zeros(3, n + 4, device=DEV)
    av, tv, gv = buf[0, 1:n + 1], buf[1, 1:n + 1], buf[2, 1:n + 1]
    av.copy_(a.view(-1)), tv.copy_(t.view(-1))
    assert av.data_ptr() % 16 == 4
    pd = torch.from_numpy(pad).to(DEV, torch.uint8).contiguous()
    dw, sw = dim_w.to(DEV), step_w.to(DEV)
    part, out = torch.zeros(768, device=DEV), torch.zeros(3, device=DEV)
    call(lib().fv_op_chunk_loss_weighted(av.data_ptr(), tv.data_ptr(), pd.data_ptr(), dw.data_ptr(), sw.data_ptr(), gv.data_ptr(), part.data_ptr(), 768,
                                         out.data_ptr(), out[1:].data_ptr(), n, A, K, KIND_ID["smooth_l1"], BETA, 1.0, stream()), "fv_op_chunk_loss_weighted")
    torch.cuda.synchronize()
    ref = weighted_loss_ref(a.numpy(), t.numpy(), pad, dim_w.numpy(), step_w.numpy(), "smooth_l1", BETA)
    _check((float(out[0]), out[1:].cpu(), gv.cpu().view(B, K, A)), ref, "unaligned")
    aligned = _op_weighted(a, t, pad, dim_w, step_w, "smooth_l1")
    assert torch.equal(gv.cpu().view(B, K, A), aligned[2])                    # the same g as the float4 body
    assert float(buf[2, 0]) == 0.0 and float(buf[2, n + 1]) == 0.0           # nothing written outside g
    # argument checks of the op: a missing vector, a chunk length that does not divide the step count
    assert lib().fv_op_chunk_loss_weighted(av.data_ptr(), tv.data_ptr(), None, None, sw.data_ptr(), gv.data_ptr(), part.data_ptr(), 768, out.data_ptr(),
                                           out[1:].data_ptr(), n, A, K, 0, 1.0, 1.0, stream()) == -1
    assert lib().fv_op_chunk_loss_weighted(av.data_ptr(), tv.data_ptr(), None, dw.data_ptr(), sw.data_ptr(), gv.data_ptr(), part.data_ptr(), 768, out.data_ptr(),
                                           out[1:].data_ptr(), n, A, 2, 0, 1.0, 1.0, stream()) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. the setters
def _step(eng, p, pooled, states, tgt, pad=None):
    flat = _flat(eng, p)
    act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
    loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved, pad=pad)
    torch.cuda.synchronize()
    return loss.clone(), grads.clone()


def _farr(v):
    return (C.c_float * len(v))(*v)


def test_setter_argument_checks_change_nothing_and_a_new_chunk_drops_the_weights():
    B, K, A = 3, 4, 5
    da = K * A
    p = _head_params(da, 3)
    pooled, states, tgt = _head_io(B, da, 4)
    eng = _head_engine(da, B)
    L = eng.lib
    eng.set_head_loss("l1", 1.0, K)
    assert eng.head_loss_weights is None
    l0, g0 = _step(eng, p, pooled, states, tgt)
    dim_w, step_w = [1.0, 2.0, 0.0, 0.5, 3.0], [1.0, 0.5, 0.25, 0.0]
    eng.set_head_loss_weights(dim_w, step_w)
    assert eng.head_loss_weights == {"dim": dim_w, "step": step_w} and eng.loss_is_chunked(None)
    l1, g1 = _step(eng, p, pooled, states, tgt)
    assert not torch.equal(g1, g0)
    ok = _farr(dim_w)
    for bad in (-1.0, float("nan"), float("inf"), float("-inf"), -1e-30):
        assert L.fv_head_set_loss_weights(eng.h, C.cast(_farr([1.0, bad, 1.0, 1.0, 1.0]), C.c_void_p), None) == -1, bad
        assert L.fv_head_set_loss_weights(eng.h, C.cast(ok, C.c_void_p), C.cast(_farr([1.0, 1.0, 1.0, bad]), C.c_void_p)) == -1, bad
    assert b"finite" in L.fv_last_error(eng.h) and L.fv_head_set_loss_weights(None, None, None) == -1
    for kw in (dict(dim_w=[1.0] * 4), dict(step_w=[1.0] * 5), dict(dim_w=[1.0, 1.0, -2.0, 1.0, 1.0]), dict(step_w=[1.0, float("nan"), 1.0, 1.0])):
        with pytest.raises(ValueError):
            eng.set_head_loss_weights(**kw)                                   # on the host, before any library call
    l2, g2 = _step(eng, p, pooled, states, tgt)
    assert torch.equal(l2, l1) and torch.equal(g2, g1)                        # every refused call left the weights as they were
    # one vector alone: the other is ones
    eng.set_head_loss_weights(dim_w, None)
    la, ga = _step(eng, p, pooled, states, tgt)
    eng.set_head_loss_weights(dim_w, [1.0] * K)
    lb, gb = _step(eng, p, pooled, states, tgt)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    # the same chunk: the weights stay; another chunk: dropped, and the loss is the unweighted one again
    eng.set_head_loss_weights(dim_w, step_w)
    eng.set_head_loss("l1", 1.0, K)
    assert eng.head_loss_weights is not None and torch.equal(_step(eng, p, pooled, states, tgt)[1], g1)
    eng.set_head_loss("l1", 1.0, 2)
    assert eng.head_loss_weights is None and eng.loss_is_chunked(None)      # (l1 runs the chunked kernel with or without weights)
    eng.set_head_loss("l1", 1.0, K)
    l3, g3 = _step(eng, p, pooled, states, tgt)
    assert torch.equal(l3, l0) and torch.equal(g3, g0)
    # ... straight through the C ABI as well (the host mirror is not what drops them)
    eng.set_head_loss_weights(dim_w, step_w)
    assert L.fv_head_set_loss(eng.h, C.byref(_lib.HeadLossSpec(1, 1.0, 2))) == 0 and L.fv_head_set_loss(eng.h, C.byref(_lib.HeadLossSpec(1, 1.0, K))) == 0
    l4, g4 = _step(eng, p, pooled, states, tgt)
    assert torch.equal(l4, l0) and torch.equal(g4, g0)
    # both NULL: off
    eng.set_head_loss_weights(dim_w, step_w)
    eng.set_head_loss_weights()
    assert eng.head_loss_weights is None and torch.equal(_step(eng, p, pooled, states, tgt)[1], g0)
    eng.close()


def test_plain_mse_with_weights_takes_the_weighted_instance_and_back():
    """kind MSE, no mask: the single-block kernel -- until weights are set; then the weighted instance (and the metrics are written); off again: the old bits"""
    B, K, A = 3, 4, 5
    da = K * A
    p = _head_params(da, 3)
    pooled, states, tgt = _head_io(B, da, 4)
    eng = _head_engine(da, B)
    eng.set_head_loss("mse", 1.0, K)
    assert not eng.loss_is_chunked(None)
    l0, g0 = _step(eng, p, pooled, states, tgt)
    dim_w, step_w = _weights(A, K, seed=2)
    eng.set_head_loss_weights(dim_w, step_w)
    assert eng.loss_is_chunked(None)
    flat = _flat(eng, p)
    act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
    loss, _ = eng.head_backward(flat, act, tgt.to(DEV), saved)
    met = eng.head_loss_metrics().cpu()
    ref = weighted_loss_ref(act.cpu().view(B, K, A).numpy(), tgt.view(B, K, A).numpy(), None, dim_w.numpy(), step_w.numpy(), "mse")
    assert abs(float(loss) - ref["loss"]) <= 1e-5 * ref["loss"] and abs(float(met[0]) - ref["mse"]) <= 1e-5 * ref["mse"] and float(met[1]) == 1.0
    eng.set_head_loss_weights()
    l1, g1 = _step(eng, p, pooled, states, tgt)
    assert torch.equal(l1, l0) and torch.equal(g1, g0)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the per-dimension error
@pytest.mark.parametrize("shape", [(3, 4, 5), (9, 7, 14)])
def test_loss_per_dim_matches_float64(shape):
    B, K, A = shape
    a, t = _loss_inputs(B, K, A, seed=B + K)
    eng = _head_engine(K * A, B)
    eng.set_head_loss("l1", 1.0, K)
    eng.set_head_loss_weights([0.0] + [1.0] * (A - 1), None)                  # the error is never weighted
    for name, pad in (("none", None), ("ragged", ragged_pad(B, K, seed=1)), ("one-step", ~np.eye(1, B * K, 3, dtype=bool).reshape(B, K))):
        got = eng.head_loss_per_dim(a.to(DEV), t.to(DEV), pad=pad).cpu().double()
        valid = np.ones((B, K), dtype=bool) if pad is None else ~pad
        ref = torch.from_numpy(np.abs(a.double().numpy() - t.double().numpy())[valid].mean(axis=0))
        assert got.shape == (A,) and bool(((got - ref).abs() <= 1e-5 * ref.abs()).all()), (name, got, ref)
    t_bad = t.clone()
    t_bad[torch.from_numpy(ragged_pad(B, K, seed=1))] = float("nan")           # what padded steps hold never enters
    got = eng.head_loss_per_dim(a.to(DEV), t_bad.to(DEV), pad=ragged_pad(B, K, seed=1))
    assert torch.equal(got, eng.head_loss_per_dim(a.to(DEV), t.to(DEV), pad=ragged_pad(B, K, seed=1)))
    assert torch.equal(got, eng.head_loss_per_dim(a.view(B, K * A).to(DEV), t.view(B, K * A).to(DEV), pad=ragged_pad(B, K, seed=1)))      # two runs, either layout
    # every step padded: no valid step in any dimension -> 0, not NaN
    none = eng.head_loss_per_dim(a.to(DEV), t_bad.to(DEV), pad=np.ones((B, K), dtype=bool))
    assert bool((none == 0).all())
    L = eng.lib
    out = torch.full((A,), 7.0, device=DEV)
    ad, td = a.to(DEV), t.to(DEV)
    assert L.fv_head_loss_per_dim(eng.h, None, td.data_ptr(), B, out.data_ptr(), stream()) == -1
    assert L.fv_head_loss_per_dim(eng.h, ad.data_ptr(), td.data_ptr(), B, None, stream()) == -1
    assert L.fv_head_loss_per_dim(eng.h, ad.data_ptr(), td.data_ptr(), 0, out.data_ptr(), stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the head step against autograd
@pytest.mark.parametrize("kind", KINDS)
def test_weighted_head_step_matches_float64_autograd(kind):
    B, K, A = 3, 4, 5
    da = K * A
    p = _head_params(da, 7)
    pooled, states, tgt = _head_io(B, da, 8)
    pad = ragged_pad(B, K, seed=1)
    dim_w, step_w = _weights(A, K, seed=6)
    eng = _head_engine(da, B)
    eng.set_head_loss(kind, BETA, K)
    eng.set_head_loss_weights(dim_w, step_w)
    flat = _flat(eng, p)
    act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
    loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved, pad=pad)
    met = eng.head_loss_metrics().cpu()
    torch.cuda.synchronize()
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    pred = head.head_forward(p64, pooled.double(), states.double()).view(B, K, A)
    om = step_w.double().view(1, K, 1) * dim_w.double().view(1, 1, A)
    import torch.nn.functional as F
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "smooth_l1": lambda x, y, reduction: F.smooth_l1_loss(x, y, reduction=reduction, beta=BETA)}[kind]
    per = fn(pred, tgt.double().view(B, K, A), reduction="none") * om
    per = torch.where(torch.from_numpy(pad).unsqueeze(-1).expand_as(per), torch.zeros_like(per), per)
    ref = per.sum() / per.numel()
    ref.backward()
    np.testing.assert_allclose(act.cpu().numpy(), pred.detach().view(B, da).numpy(), rtol=1e-4, atol=1e-5)
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    r = weighted_loss_ref(pred.detach().numpy(), tgt.view(B, K, A).numpy(), pad, dim_w.numpy(), step_w.numpy(), kind, BETA)
    assert abs(float(met[0]) - r["mse"]) <= 1e-5 * r["mse"] and abs(float(met[1]) - float((~pad).mean())) <= 1e-6
    gv = eng.head_views(grads)
    worst = 0.0
    for k in HEAD_KEYS:
        rr = p64[k].grad
        bar = 2e-5 * max(1e-3, float(rr.abs().max()))
        err = float((gv[k].cpu().double() - rr).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (k, err, bar)
    print(f"[weighted head step {kind}] worst gradient error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. through the policy, every route
def _policy(model, K, frozen=True, **kw):
    torch.manual_seed(31)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{model}", hidden_dim=48, fusion_dim=64, dropout=0.0, freeze_backbone=frozen), chunk_size=K,
                         action_loss="l1", **kw).to(DEV)


ROUTES = {"head-only": ("tiny:77", None), "lora": ("small:43", dict(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"])),
          "lora-direct": ("small:43", dict(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"], lora_direct=True)),
          "full": ("small:43", dict())}


@pytest.mark.parametrize("route", list(ROUTES))
def test_targets_of_zero_weight_elements_change_no_bit(route):
    """One train step twice from the same initialisation; the second batch's targets differ -- by finite values, NaN and inf -- in a zero-weight dimension and a
    zero-weight step only: the loss and EVERY gradient keep their bits.  Head-only on synthetic:tiny; the backbone-training routes (full, LoRA projected,
    LoRA direct) on synthetic:small, the smallest preset the training kernels take (they need a decoder head_dim of 64 or 128; tiny's is 32)."""
    model, train = ROUTES[route]
    K, A, B = 4, 14, 3
    dim_w, step_w = [1.0] * (A - 1) + [0.0], [1.0, 0.5, 0.0, 0.25]
    batch = _chunk_batch(B, K, pads=[0, 1, 0])
    other = {**batch, "actions": batch["actions"].clone()}
    other["actions"][:, :, A - 1] += 3.0
    other["actions"][:, 2, :] = torch.tensor([float("nan"), float("inf"), -5.0, float("-inf")]).repeat(B * A)[: B * A].view(B, A)
    kw = dict(lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    seen = []
    for b in (batch, other, batch):
        pol = _policy(model, K, frozen=train is None, action_dim_weights=dim_w, action_step_weights=step_w)
        if train is not None:
            pol.enable_backbone_training(**train)
        pol.train()
        out = pol.fused_train_step(_dev(b), **kw)
        torch.cuda.synchronize()
        un = pol._unfrozen
        g = pol._opt_state["g"] if un is None else (un.lg if un.lora is not None else un.g)
        assert torch.isfinite(out["loss"]) and torch.isfinite(g).all() and float(g.abs().max()) > 0
        seen.append((out["loss"].clone(), g.clone(), out["grad_norm"].clone(), out["mse"].clone()))
        assert pol.model.backbone.engine().loss_is_chunked(None)
        pol.model.backbone.engine().close()
    (l0, g0, n0, m0), (l1, g1, n1, m1), (l2, g2, n2, m2) = seen
    assert torch.equal(l2, l0) and torch.equal(g2, g0)                        # (the step itself repeats bit for bit)
    assert torch.equal(l1, l0) and torch.equal(g1, g0) and torch.equal(n1, n0) and torch.equal(m1, m0)
    # ... and the weights do reach this route: without them the same step gives another gradient
    pol = _policy(model, K, frozen=train is None)
    if train is not None:
        pol.enable_backbone_training(**train)
    pol.train()
    out = pol.fused_train_step(_dev(batch), **kw)
    torch.cuda.synchronize()
    un = pol._unfrozen
    g = pol._opt_state["g"] if un is None else (un.lg if un.lora is not None else un.g)
    assert not torch.equal(g, g0) and not torch.equal(out["loss"], l0)
    pol.model.backbone.engine().close()


def test_policy_surfaces():
    K, A, B = 4, 14, 3
    batch = _dev(_chunk_batch(B, K, pads=[0, 1, 0]))
    plain = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K).to(DEV)
    eng = plain.model.backbone.engine()
    assert eng.head_loss_weights is None and not eng.loss_is_chunked(None) and eng.loss_is_chunked(batch["action_is_pad"])      # as before: MSE is chunked with a mask only
    nomask = {k: v for k, v in batch.items() if k != "action_is_pad"}
    out = plain.compute_loss(nomask)
    assert plain.model.last_loss_metrics is None and torch.equal(out["mse"], out["loss"].detach())
    # action_error_per_dim: the float64 mean |d| of the policy's own normalised predictions
    err = plain.action_error_per_dim(batch).cpu().double()
    pred = plain.forward(batch["images"], batch["states"], batch["tasks"]).detach().cpu().double()
    valid = ~batch["action_is_pad"].cpu().numpy()
    ref = torch.from_numpy(np.abs(pred.numpy() - batch["actions"].cpu().double().numpy())[valid].mean(axis=0))
    assert err.shape == (A,) and bool(((err - ref).abs() <= 1e-5 * ref).all())
    # set_action_loss_weights on a live engine: compute_loss follows the float64 definition, the masked MSE stays unweighted
    dim_w, step_w = [1.0] * (A - 1) + [4.0], [1.0, 0.5, 0.25, 0.0]
    plain.set_action_loss_weights(dim_w, step_w)
    out = plain.compute_loss(batch)
    r = weighted_loss_ref(pred.numpy(), batch["actions"].cpu().numpy(), batch["action_is_pad"].cpu().numpy(), dim_w, step_w, "mse")
    assert abs(float(out["loss"].detach()) - r["loss"]) <= 1e-5 * r["loss"] and abs(float(out["mse"]) - r["mse"]) <= 1e-5 * r["mse"]
    out["loss"].backward()
    assert plain.model.action_head.weight.grad is not None
    with pytest.raises(ValueError):
        plain.set_action_loss_weights([1.0] * (A + 1))
    plain.set_action_loss_weights()
    assert not eng.loss_is_chunked(None)
    eng.close()
    # the LeRobot surface
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    A = 5
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=1,
                   output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
    torch.manual_seed(3)
    dim_w, step_w = [1.0, 1.0, 1.0, 1.0, 0.0], [1.0, 0.5, 0.25, 0.125]
    pol = LRPolicy(cfg, action_dim_weights=dim_w, action_step_weights="discount:0.5").to(DEV)
    g = torch.Generator().manual_seed(4)
    tgt, pad = torch.randn(2, K, A, generator=g), torch.from_numpy(ragged_pad(2, K, seed=2))
    lb = {"observation.images.top": torch.rand(2, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(2, 6, generator=g).to(DEV), "task": ["a", "b"],
          ACTION: tgt.to(DEV), "action_is_pad": pad.to(DEV)}
    pol.train()
    loss, info = pol.forward(lb)
    with torch.no_grad():
        _, pred = pol.model.forward_loss(lb["observation.images.top"], lb["observation.state"], ["a\n", "b\n"], tgt.to(DEV), pad=pad.to(DEV))
    r = weighted_loss_ref(pred.cpu().numpy(), tgt.numpy(), pad.numpy(), dim_w, step_w, "mse")
    assert abs(float(loss.detach()) - r["loss"]) <= 1e-5 * r["loss"] and abs(info["mse"] - r["mse"]) <= 1e-5 * r["mse"]
    err = pol.action_error_per_dim(lb).cpu().double()
    ref = torch.from_numpy(np.abs(pred.cpu().double().numpy() - tgt.double().numpy())[~pad.numpy()].mean(axis=0))
    assert bool(((err - ref).abs() <= 1e-5 * ref).all())
    pol.model.backbone.engine().close()
