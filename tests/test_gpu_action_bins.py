"""-m gpu: the binned action head -- the loss and decode kernels against float64 (tests/action_bins_util.py), their exact rules, the head step against
autograd, the setter's rules, and the policy level on synthetic:tiny:77 (training, select_action, temporal ensembling, backbone training, the step guard,
checkpoints and Trainer resume).

Bars.  Op level, from fp32 rounding of a max-subtracted softmax over <= 1024 terms: every gradient element within 4e-6 loss_scale om / n of float64, the loss
within 1e-5 absolute, the "mean" decode within 4e-6 max(|lo|, |hi|).  The decoded squared error of the metrics inherits the decode's bound: a term
(dec - t)^2 moves by at most 2 |dec - t| delta, delta the decode's bound ("argmax": the fp32 rounding of the centre, 2^-23 max(|lo|, |hi|)), plus the fp32 sum's
1e-6 of the value.  The valid fraction and the accuracy are quotients of two small integers: the fp32 quotient exactly.  Head level: the project's own bars of
test_gpu_action_chunk.py (loss relative 1e-5, head gradients 2e-5 max(1e-3, max|ref|) per tensor; backbone gradients rel_l2 GRAD_TOL)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from action_bins_util import bins_ref, bins_table, make_targets, per_element, torch_bins_loss  # noqa: E402
from chunk_loss_util import ragged_pad  # noqa: E402
from gpu_util import DEV, call, lib, rel_l2, stream  # noqa: E402
from fastvla_hip import HEAD_KEYS, FastVLAEngine, FastVLAHipError, _lib, arch, weights  # noqa: E402
from oracle import head, qwen2, train_unfrozen  # noqa: E402
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy  # noqa: E402

DECODE = _lib.BINS_DECODES
C_f = C.c_float
SHAPES = [(1, 1, 1, 2), (3, 2, 5, 64), (2, 3, 3, 96), (5, 1, 7, 256), (2, 2, 3, 1024), (9, 4, 14, 256)]


def _ranges(A, nb):
    """(-3, 3) for everything at 96 bins (w = 1/16 exactly); otherwise one pair per action dimension, cycling through a few spans"""
    if nb == 96:
        return [(-3.0, 3.0)]
    base = [(-3.0, 3.0), (-1.0, 1.0), (-0.7, 2.3), (0.0, 1.5), (-2.5, -0.5)]
    return [base[a % len(base)] for a in range(A)]


def _dev_table(table):
    return torch.from_numpy(np.concatenate(table)).to(DEV).contiguous()


def _op_loss(z, t, table, pad=None, sigma=0.0, decode="argmax", dim_w=None, step_w=None, loss_scale=1.0, misalign=False):
    """bins_loss_kernel + fold alone (fv_op_bins_loss): z (B, K, A, Nb), t (B, K, A) f32 CPU -> loss, metrics (4,), g (B, K, A, Nb) on the CPU (+ the floats
    around g when misalign: logits and g then start 4 bytes off a 16-byte boundary)"""
    B, K, A, nb = z.shape
    n = B * K * A
    off = 1 if misalign else 0
    zbuf, gbuf = torch.zeros(z.numel() + 8, device=DEV), torch.full((z.numel() + 8,), 7.0, device=DEV)
    zd, gd = zbuf[off:off + z.numel()], gbuf[off:off + z.numel()]
    zd.copy_(z.reshape(-1))
    assert zd.data_ptr() % 16 == 4 * off and gd.data_ptr() % 16 == 4 * off
    td = t.to(DEV).contiguous()
    pd = None if pad is None else torch.as_tensor(pad).to(DEV, torch.uint8).contiguous()
    dw = None if dim_w is None else torch.tensor(dim_w, dtype=torch.float32, device=DEV)
    sw = None if step_w is None else torch.tensor(step_w, dtype=torch.float32, device=DEV)
    rng = _dev_table(table)
    nblk = (n + 3) // 4
    part, out = torch.full((4 * nblk,), float("nan"), device=DEV), torch.full((5,), float("nan"), device=DEV)
    call(lib().fv_op_bins_loss(zd.data_ptr(), td.data_ptr(), None if pd is None else pd.data_ptr(), None if dw is None else dw.data_ptr(),
                               None if sw is None else sw.data_ptr(), rng.data_ptr(), len(table[0]), sigma, DECODE[decode], gd.data_ptr(), part.data_ptr(), part.numel(),
                               out.data_ptr(), out[1:].data_ptr(), n, nb, K * A, K, loss_scale, stream()), "fv_op_bins_loss")
    torch.cuda.synchronize()
    if misalign:
        assert float(gbuf[0]) == 7.0 and bool((gbuf[off + z.numel():] == 7.0).all())      # nothing written outside g
    return float(out[0]), out[1:].cpu(), gd.cpu().view(B, K, A, nb).clone()


def _op_decode(z, table, decode, post=None, probs=False, misalign=False):
    """bins_decode_kernel alone (fv_op_bins_decode): z (B, K, A, Nb) f32 CPU -> actions (B, K, A) [, probs (B, K, A, Nb)] on the CPU"""
    B, K, A, nb = z.shape
    n = B * K * A
    off = 1 if misalign else 0
    zbuf = torch.zeros(z.numel() + 8, device=DEV)
    zd = zbuf[off:off + z.numel()]
    zd.copy_(z.reshape(-1))
    act = torch.full((n,), float("nan"), device=DEV)
    pr = torch.full((z.numel() + 8,), float("nan"), device=DEV) if probs else None
    prv = None if pr is None else pr[off:off + z.numel()]
    sc, sh = (None, None) if post is None else (post[0].to(DEV).contiguous(), post[1].to(DEV).contiguous())
    rng = _dev_table(table)
    call(lib().fv_op_bins_decode(zd.data_ptr(), rng.data_ptr(), len(table[0]), DECODE[decode], act.data_ptr(), None if prv is None else prv.data_ptr(), n, nb, K * A,
                                 None if sc is None else sc.data_ptr(), None if sh is None else sh.data_ptr(), stream()), "fv_op_bins_decode")
    torch.cuda.synchronize()
    a = act.cpu().view(B, K, A)
    return (a, prv.cpu().view(B, K, A, nb).clone()) if probs else a


def _inputs(shape, seed=None):
    B, K, A, nb = shape
    g = torch.Generator().manual_seed(B * 1000 + K * 100 + A * 10 + nb if seed is None else seed)
    z = (torch.rand(B, K, A, nb, generator=g) * 16.0 - 8.0)
    table = bins_table(_ranges(A, nb), nb, K * A)
    t = make_targets(B, K, A, table, nb, seed=nb + B)
    return z, t, table


def _weights(K, A):
    dw = [0.5 + 0.25 * (a % 5) for a in range(A)]
    sw = [1.0 / (1 + k) for k in range(K)]
    if A > 1:
        dw[A - 1] = 0.0                                                       # one dimension is weighted out altogether
    return dw, sw


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels against float64
@pytest.mark.parametrize("sigma", [0.0, 0.75])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_loss_kernel_matches_float64(shape, sigma):
    B, K, A, nb = shape
    z, t0, table = _inputs(shape)
    n = B * K * A
    rag = ragged_pad(B, K, seed=1) if B * K > 1 else None
    worst = {"g": 0.0, "loss": 0.0, "sqerr": 0.0}
    lo, hi, _w = per_element(table, K, A)
    top = np.maximum(np.abs(lo), np.abs(hi))
    for pad in ((None,) if rag is None else (None, rag)):
        for weighted in (False, True):
            dw, sw = _weights(K, A) if weighted else (None, None)
            t = t0.clone()
            if pad is not None:                                               # what a padded step holds must not matter
                sel = torch.from_numpy(pad).unsqueeze(-1).expand_as(t)
                t[sel] = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(int(sel.sum())) % 3]
            if weighted and A > 1:
                t[:, :, A - 1] = float("nan")                                 # nor what a zero-weight element holds
            for decode, ls in (("argmax", 1.0), ("mean", 1024.0)):
                loss, met, g = _op_loss(z, t, table, pad, sigma, decode, dw, sw, ls)
                ref = bins_ref(z.numpy(), t.numpy(), table, pad, sigma, decode, dw, sw, ls)
                print(f"[bins loss {shape} sigma={sigma} pad={pad is not None} weighted={weighted} {decode}] loss {loss!r} ref {ref['loss']!r} metrics {met.tolist()}")
                assert np.isfinite(loss) and bool(torch.isfinite(met).all()) and bool(torch.isfinite(g).all())
                bar = 4e-6 * ls * ref["om"][None, :, :, None] / n
                err = np.abs(g.double().numpy() - ref["g"])
                live = ref["live"]
                if live.any():
                    worst["g"] = max(worst["g"], float((err[live] / np.broadcast_to(bar, err.shape)[live]).max()))
                assert bool((err <= bar).all()), ("g", float((err / np.maximum(bar, 1e-300)).max()))
                assert bool((g[torch.from_numpy(~live)] == 0).all())           # selected away: all Nb elements exactly 0
                worst["loss"] = max(worst["loss"], abs(loss - ref["loss"]) / 1e-5)
                assert abs(loss - ref["loss"]) <= 1e-5, ("loss", loss, ref["loss"])
                delta = 4e-6 * top if decode == "mean" else 2.0 ** -23 * top
                sq_bar = float((2.0 * ref["abs_d"] * delta[None]).sum() / n) + 1e-6 * ref["sqerr"] + 1e-12
                worst["sqerr"] = max(worst["sqerr"], abs(float(met[0]) - ref["sqerr"]) / sq_bar)
                assert abs(float(met[0]) - ref["sqerr"]) <= sq_bar, ("sqerr", float(met[0]), ref["sqerr"], sq_bar)
                nvalid_f = np.float32(ref["nvalid"])
                assert float(met[1]) == float(nvalid_f / np.float32(n)) and float(met[3]) == 0.0
                assert float(met[2]) == (float(np.float32(ref["hits"]) / nvalid_f) if ref["nvalid"] else 0.0)
                if decode == "mean":                                          # the decode kernel on the same logits
                    dec = _op_decode(z, table, "mean")
                    derr = np.abs(dec.double().numpy() - ref["decoded"])
                    assert bool((derr <= 4e-6 * top[None]).all()), ("mean decode", float((derr / (4e-6 * top[None])).max()))
    print(f"[bins loss {shape} sigma={sigma}] worst error / bar: g {worst['g']:.3f} loss {worst['loss']:.3f} decoded sq. error {worst['sqerr']:.3f}")
    if rag is not None:                                                       # all padded: exactly nothing
        loss, met, g = _op_loss(z, t0, table, np.ones((B, K), dtype=bool), sigma)
        assert loss == 0.0 and bool((met == 0).all()) and bool((g == 0).all())


@pytest.mark.parametrize("shape", [(3, 2, 5, 64), (5, 1, 7, 256), (2, 2, 3, 1024)], ids=str)
def test_two_runs_agree_bit_for_bit(shape):
    B, K, A, nb = shape
    z, t, table = _inputs(shape)
    dw, sw = _weights(K, A)
    pad = ragged_pad(B, K, seed=1)
    for sigma in (0.0, 0.75):
        r1, r2 = (_op_loss(z, t, table, pad, sigma, "mean", dw, sw, 4.0) for _ in range(2))
        assert r1[0] == r2[0] and torch.equal(r1[1], r2[1]) and torch.equal(r1[2].view(torch.int32), r2[2].view(torch.int32))
    d1, d2 = (_op_decode(z, table, "mean", probs=True) for _ in range(2))
    assert torch.equal(d1[0], d2[0]) and torch.equal(d1[1], d2[1])


@pytest.mark.parametrize("nb", [2, 64, 256, 1024])
def test_equal_logits_give_exactly_one_over_nb(nb):
    """exp(0) = 1 exactly, the sum of Nb ones is Nb exactly, and 1 / Nb is exact for a power of two"""
    z = torch.full((2, 1, 3, nb), 1.625)
    table = bins_table((-1.0, 1.0), nb, 3)
    act, p = _op_decode(z, table, "mean", probs=True)
    assert bool((p == 1.0 / nb).all())
    assert bool((act.abs() <= 1e-6).all())                                    # the mean of the centres of a symmetric range
    assert torch.equal(_op_decode(z, table, "argmax"), torch.full((2, 1, 3), float(np.float32(-1.0) + np.float32(0.5) * table[2][0])))      # every bin ties: the lowest index


@pytest.mark.parametrize("nb,rng", [(2, (-1.0, 1.0)), (64, (-1.0, 1.0)), (96, (-3.0, 3.0)), (256, (-2.0, 2.0)), (1024, (-4.0, 4.0))])
def test_argmax_is_the_exact_fp32_centre_with_ties_to_the_lowest_index(nb, rng):
    """ranges whose w is exact in fp32 (a power of two, or 1/16): lo + (j + 1/2) w is then exact too, and the kernel's fma gives that number"""
    table = bins_table(rng, nb, 1)
    lo, w = float(table[0][0]), float(table[2][0])
    assert w == (rng[1] - rng[0]) / nb
    g = torch.Generator().manual_seed(nb)
    G = 40
    z = torch.rand(G, 1, 1, nb, generator=g) * 4.0 - 2.0
    want = torch.empty(G, dtype=torch.int64)
    for i in range(G):
        j = int(torch.randint(0, nb, (1,), generator=g))
        js = sorted({j, (j * 7 + 3) % nb, nb - 1 - (i % nb), (j + 64) % nb, (j + 1) % nb})[: 1 + i % 4]      # 1 .. 4 tied maxima: other lanes, other registers, neighbours
        z[i, 0, 0, js] = 3.0
        want[i] = min(js)
    act = _op_decode(z, table, "argmax").view(G)
    centres = torch.tensor([lo + (int(j) + 0.5) * w for j in want], dtype=torch.float64)
    assert bool((centres.float().double() == centres).all())                  # exact in fp32 by construction
    assert torch.equal(act.double(), centres)
    # the folded action statistics behind the decode: centre * std + mean, one fp32 multiply and add
    std, mean = torch.tensor([1.75]), torch.tensor([-0.375])
    post = _op_decode(z, table, "argmax", post=(std, mean)).view(G)
    assert torch.equal(post, centres.float() * std + mean)
    # the loss kernel's accuracy and decoded error use the same argmax: targets at those centres are all hits with zero error
    loss, met, _ = _op_loss(z, centres.float().view(G, 1, 1), table)
    assert float(met[0]) == 0.0 and float(met[1]) == 1.0 and float(met[2]) == 1.0


@pytest.mark.parametrize("nb", [2, 96, 256])
def test_a_logit_of_1e4_stays_finite(nb):
    z = torch.zeros(2, 1, 2, nb)
    z[0, 0, 0, nb - 1] = 1e4
    z[1, 0, 1, 0] = 1e4
    z[1, 0, 0, :] = -1e4
    table = bins_table((-3.0, 3.0), nb, 2)
    t = torch.tensor([[[2.9, 0.1]], [[-0.3, 2.0]]])
    for sigma in (0.0, 0.75):
        loss, met, g = _op_loss(z, t, table, sigma=sigma, decode="mean")
        ref = bins_ref(z.numpy(), t.numpy(), table, sigma=sigma, decode="mean")
        assert np.isfinite(loss) and bool(torch.isfinite(met).all()) and bool(torch.isfinite(g).all())
        assert abs(loss - ref["loss"]) <= 1e-6 * max(1.0, ref["loss"])       # (a loss of ~1e4 / n: fp32 holds it to 1e-7 of its size)
        assert bool((np.abs(g.double().numpy() - ref["g"]) <= 4e-6 / 4).all())
    act, p = _op_decode(z, table, "mean", probs=True)
    assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(p).all())
    assert float(p[0, 0, 0, nb - 1]) == 1.0 and float(p[1, 0, 1, 0]) == 1.0 and bool((p[1, 0, 0] == 1.0 / nb).all() if nb & (nb - 1) == 0 else True)


@pytest.mark.parametrize("shape", [(3, 2, 5, 64), (2, 3, 3, 96), (5, 1, 7, 256), (2, 2, 3, 1024)], ids=str)
def test_gradient_of_a_group_sums_to_zero(shape):
    """sum_j (p_j - q_j) = 0.  In fp32 the sum of the stored elements is c (sum_j fl(p_j) - 1) up to their own rounding: the softmax's sum is nreg <= 16 lane
    additions and 6 butterfly steps, the division one more rounding per term -- under 24 roundings of 2^-24, relative to 1.  A hard target's own element is
    c (p_t - 1); for a group with p_t <= 1/2 it is at least c / 2, one ulp of it at least c 2^-25, so the sum stays within 48 ulps of the largest term, below
    Nb for every Nb >= 64.  (With two bins the three roundings of the two terms already exceed 2 ulps: the bound says nothing there and is not asserted.)"""
    B, K, A, nb = shape
    z, t, table = _inputs(shape)
    _, _, g = _op_loss(z, t, table)
    ref = bins_ref(z.numpy(), t.numpy(), table)
    pt = np.take_along_axis(ref["p"], ref["idx"][..., None], -1)[..., 0]
    ok = pt <= 0.5
    assert ok.mean() >= 0.9                                                   # uniform logits over >= 64 bins: nearly every target's bin holds little mass
    s = np.abs(g.double().numpy().sum(-1))
    ulp = np.spacing(np.abs(g.numpy()).max(-1)).astype(np.float64)
    print(f"[bins gradient sum {shape}] worst |sum| / ulp of the largest term: {float((s / ulp)[ok].max()):.1f} (bar {nb})")
    assert bool((s[ok] <= nb * ulp[ok]).all())


@pytest.mark.parametrize("nb", [96, 256, 1024])
def test_misaligned_pointers_take_the_scalar_form_and_give_the_same_values(nb):
    """logits, g and probs 4 bytes off a 16-byte boundary: no 16-byte access; the bin-to-lane mapping and with it every sum's order stay, so the bits do too"""
    shape = (2, 2, 3, nb)
    z, t, table = _inputs(shape, seed=77)
    dw, sw = _weights(2, 3)
    pad = ragged_pad(2, 2, seed=1)
    for sigma in (0.0, 0.75):
        a = _op_loss(z, t, table, pad, sigma, "mean", dw, sw, 2.0)
        b = _op_loss(z, t, table, pad, sigma, "mean", dw, sw, 2.0, misalign=True)
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    for decode in ("argmax", "mean"):
        a, b = _op_decode(z, table, decode, probs=True), _op_decode(z, table, decode, probs=True, misalign=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_op_argument_checks_enqueue_nothing():
    z, t, table = _inputs((2, 1, 3, 64))
    zd, td, rng = z.to(DEV), t.to(DEV), _dev_table(table)
    g, part, out = torch.full((z.numel(),), 5.0, device=DEV), torch.zeros(8, device=DEV), torch.full((5,), 5.0, device=DEV)
    L = lib()

    def loss(nb=64, da=3, K=1, n_range=3, sigma=0.0, decode=0, n=6, pf=8, dw=None, sw=None):
        return L.fv_op_bins_loss(zd.data_ptr(), td.data_ptr(), None, dw, sw, rng.data_ptr(), n_range, sigma, decode, g.data_ptr(), part.data_ptr(), pf, out.data_ptr(),
                                 out[1:].data_ptr(), n, nb, da, K, 1.0, stream())

    assert loss() == 0
    torch.cuda.synchronize()
    g.fill_(5.0), out.fill_(5.0)
    for kw in (dict(nb=1), dict(nb=1025), dict(n=5), dict(n=0), dict(n_range=2), dict(n_range=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(decode=2), dict(K=2),
               dict(pf=4), dict(dw=td.data_ptr())):
        assert loss(**kw) == -1, kw
    act = torch.full((6,), 5.0, device=DEV)
    assert L.fv_op_bins_decode(zd.data_ptr(), rng.data_ptr(), 3, 2, act.data_ptr(), None, 6, 64, 3, None, None, stream()) == -1
    assert L.fv_op_bins_decode(zd.data_ptr(), rng.data_ptr(), 3, 0, None, None, 6, 64, 3, None, None, stream()) == -1
    assert L.fv_op_bins_decode(zd.data_ptr(), rng.data_ptr(), 3, 0, act.data_ptr(), None, 6, 64, 3, td.data_ptr(), None, stream()) == -1
    torch.cuda.synchronize()
    assert bool((g == 5.0).all()) and bool((out == 5.0).all()) and bool((act == 5.0).all())


# ------------------------------------------------------------------------------------------------------------------ 2. the head
FEAT, HID, FUS, DS = 48, 24, 40, 6


def _head_engine(da, B):
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=FEAT, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    return FastVLAEngine(m, state_dim=DS, action_dim=da, hidden_dim=HID, fusion_dim=FUS, max_batch=max(B, 1))


def _head_params(width, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = head.head_shapes(FEAT, DS, width, HID, FUS)
    return {k: torch.randn(*s, generator=g) * (0.2 if len(s) > 1 else 0.1) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
            for k, s in shapes.items()}


def _flat(eng, p):
    flat = torch.zeros(eng.head_numel(), device=DEV)
    for k, v in eng.head_views(flat).items():
        v.copy_(p[k])
    return flat


def _head_io(B, da, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, FEAT, generator=g), torch.randn(B, DS, generator=g)


@pytest.mark.parametrize("sigma,decode", [(0.0, "argmax"), (0.75, "mean")])
def test_head_step_matches_float64_autograd(sigma, decode):
    """forward, loss and all 12 gradients of one head step (the dimensions and bars of test_gpu_action_chunk.py's test_head_step_matches_float64_autograd),
    24 bins per element -- ragged lanes --, a range per action dimension, a ragged mask and weights"""
    B, K, A, nb = 3, 4, 5, 24
    da = K * A
    ranges = _ranges(A, nb)
    table = bins_table(ranges, nb, da)
    p = _head_params(da * nb, 7)
    pooled, states = _head_io(B, da, 8)
    tgt = make_targets(B, K, A, table, nb, seed=9)
    pad = ragged_pad(B, K, seed=1)
    dw, sw = _weights(K, A)
    eng = _head_engine(da, B)
    eng.set_head_bins(nb, ranges, sigma, decode)
    assert eng.head_numel() > da * nb * FUS and eng.head_views(torch.zeros(eng.head_numel()))["action_head.weight"].shape == (da * nb, FUS)
    eng.set_head_loss("mse", 1.0, K)
    eng.set_head_loss_weights(dw, sw)
    flat = _flat(eng, p)
    act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV), normalized_actions=True)
    loss, grads = eng.head_backward(flat, act, tgt.view(B, da).to(DEV), saved, pad=pad)
    met = eng.head_loss_metrics().cpu()
    logits = eng.head_bins_logits(saved, B).cpu()
    probs = eng.head_bins_probs(saved, B).cpu()
    torch.cuda.synchronize()
    assert act.shape == (B, da) and logits.shape == (B, da, nb) and met.shape == (3,)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    z64 = head.head_forward(p64, pooled.double(), states.double()).view(B, K, A, nb)          # the unchanged oracle head, K * A * Nb wide
    ref = torch_bins_loss(z64, tgt, table, torch.from_numpy(pad), sigma, dw, sw)
    ref.backward()
    np.testing.assert_allclose(logits.numpy().reshape(B, K, A, nb), z64.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(probs.numpy().reshape(B, K, A, nb), torch.softmax(z64.detach(), -1).numpy(), rtol=1e-4, atol=1e-6)
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    # decode and metrics: float64 of the DEVICE's logits (an argmax must not hang on the last bit of a logit)
    r = bins_ref(logits.double().numpy().reshape(B, K, A, nb), tgt.numpy(), table, pad, sigma, decode, dw, sw)
    np.testing.assert_allclose(act.cpu().numpy().reshape(B, K, A), r["decoded"], rtol=0, atol=4e-6 * 3.0)
    sq_bar = float((2.0 * r["abs_d"] * 4e-6 * 3.0).sum() / (B * da)) + 1e-6 * r["sqerr"] + 1e-12      # (the op-level bar: the decode's bound through 2 |d|)
    assert abs(float(met[0]) - r["sqerr"]) <= sq_bar and float(met[1]) == float(np.float32(r["nvalid"]) / np.float32(B * da))
    assert float(met[2]) == float(np.float32(r["hits"]) / np.float32(r["nvalid"]))
    gv = eng.head_views(grads)
    worst = 0.0
    for k in HEAD_KEYS:
        rg = p64[k].grad
        bar = 2e-5 * max(1e-3, float(rg.abs().max()))
        err = float((gv[k].cpu().double() - rg).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (k, err, bar)
    print(f"[bins head step sigma={sigma} {decode}] worst gradient error / bar {worst:.3f}; loss {float(loss)!r} vs {float(ref.detach())!r}")
    # inference form: the folded action statistics behind the decode
    std, mean = torch.rand(A) + 0.5, torch.randn(A)
    eng.set_io_norm(torch.zeros(DS), torch.ones(DS), mean.repeat(K), std.repeat(K), eps=0.0)
    raw, _ = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
    np.testing.assert_allclose(raw.cpu().numpy(), (act.cpu() * std.repeat(K) + mean.repeat(K)).numpy(), rtol=1e-6, atol=1e-6)      # (one fma against a multiply and an add)
    # all padded: loss 0.0 and every one of the 12 gradients exactly zero
    loss0, g0 = eng.head_backward(flat, act, tgt.view(B, da).to(DEV), saved, pad=np.ones((B, K), dtype=bool))
    torch.cuda.synchronize()
    assert float(loss0) == 0.0 and all(bool((v == 0).all()) for v in eng.head_views(g0).values())
    eng.close()


def test_set_bins_then_null_leaves_the_regression_handle_its_bits():
    B, K, A = 3, 2, 5
    da = K * A
    p = _head_params(da, 3)
    pooled, states = _head_io(B, da, 4)
    tgt = torch.randn(B, da, generator=torch.Generator().manual_seed(5))
    fresh, seen = _head_engine(da, B), _head_engine(da, B)

    def step(eng):
        flat = _flat(eng, p)
        act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV))
        loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved)
        torch.cuda.synchronize()
        return act.clone(), loss.clone(), grads.clone(), saved.numel()

    n0, ws0 = fresh.head_numel(), fresh.workspace_bytes(B, 1, False)
    seen.set_head_bins(64, [(-1.0, 1.0)] * A, 0.75, "mean")
    wide = seen.head_views(torch.zeros(seen.head_numel()))
    assert tuple(wide["action_head.weight"].shape) == (da * 64, FUS) and tuple(wide["action_head.bias"].shape) == (da * 64,)
    assert seen.head_offsets[:11] == fresh.head_offsets[:11] and seen.head_numel() > n0 and seen.workspace_bytes(B, 1, False) > ws0
    seen.set_head_bins(None)
    assert seen.head_numel() == n0 and seen.head_offsets == fresh.head_offsets and seen.workspace_bytes(B, 1, False) == ws0 and seen.head_bins is None
    a, b = step(fresh), step(seen)
    assert a[3] == b[3] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3]))
    with pytest.raises(ValueError):
        seen.head_bins_logits(torch.zeros(4, device=DEV), B)
    fresh.close(), seen.close()


def test_setter_rules_and_refusals_enqueue_nothing():
    eng = _head_engine(20, 2)
    L = eng.lib
    lo, hi = (C_f * 4)(-1.0, -1.0, -1.0, -1.0), (C_f * 4)(1.0, 1.0, 1.0, 1.0)
    n0 = eng.head_numel()

    def rc(bins=16, decode=0, sigma=0.0, n_range=1, lo_=lo, hi_=hi):
        return L.fv_head_set_bins(eng.h, _lib.HeadBinsSpec(bins, decode, sigma, n_range), lo_, hi_)

    bad_lo, bad_hi = (C_f * 4)(-1.0, 1.0, float("nan"), 0.0), (C_f * 4)(1.0, 1.0, 1.0, float("inf"))
    for kw in (dict(bins=1), dict(bins=1025), dict(decode=2), dict(decode=-1), dict(sigma=-0.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(n_range=0),
               dict(n_range=3), dict(n_range=40), dict(n_range=2, lo_=bad_lo), dict(n_range=4, lo_=bad_lo), dict(n_range=4, hi_=bad_hi), dict(lo_=None), dict(hi_=None),
               dict(lo_=hi, hi_=lo), dict(bins=1024, n_range=1)):             # the last: 20 * 1024 = 20480 fits; see below
        want = 0 if kw == dict(bins=1024, n_range=1) else -1
        assert rc(**kw) == want, kw
        if want == 0:
            assert L.fv_head_set_bins(eng.h, None, None, None) == 0
        offs = (C.c_int64 * 13)()
        assert L.fv_head_layout(eng.h, offs) == 0 and offs[12] == n0, kw      # a refusal changes nothing
    wide = _head_engine(40, 2)
    assert L.fv_head_set_bins(wide.h, _lib.HeadBinsSpec(1024, 0, 0.0, 1), lo, hi) == -1 and "32768" in L.fv_last_error(wide.h).decode()      # 40 * 1024 = 40960
    assert L.fv_head_set_bins(wide.h, _lib.HeadBinsSpec(819, 0, 0.0, 1), lo, hi) == 0                                                        # 40 * 819 = 32760
    wide.close()
    assert L.fv_head_set_bins(None, None, None, None) == -1
    # bins and flow exclude each other, both ways
    eng.set_head_bins(16, (-1.0, 1.0))
    assert L.fv_head_set_flow(eng.h, _lib.HeadFlowSpec(8, 4e-3, 4.0, 0, 0.0, 1.0)) == -2 and "bins" in L.fv_last_error(eng.h).decode()
    eng.set_head_bins(None)
    eng.set_head_flow(time_dim=8)
    assert rc() == -2 and "flow" in L.fv_last_error(eng.h).decode()
    eng.set_head_flow(None)
    # the loss kind has no meaning for a bins head; a caller's grad_actions is refused; both before anything is enqueued
    eng.set_head_bins(16, (-1.0, 1.0))
    flat = torch.zeros(eng.head_numel(), device=DEV)
    act, saved = eng.head_forward(flat, torch.zeros(2, FEAT, device=DEV), torch.zeros(2, DS, device=DEV), normalized_actions=True)
    assert bool((act == float(np.float32(-1.0) + np.float32(0.5) * np.float32(0.125))).all())      # all-zero parameters: every bin ties, the lowest centre
    eng.set_head_loss("l1", 1.0, 4)
    grads = torch.full((eng.head_numel(),), 3.0, device=DEV)
    with pytest.raises(FastVLAHipError, match="loss kind") as ei:
        eng.head_backward(flat, act, torch.zeros(2, 20, device=DEV), saved, flat_grads=grads)
    assert ei.value.status == -2
    with pytest.raises(FastVLAHipError, match="bins head") as ei:
        eng.head_backward_from_grad(flat, torch.zeros(2, 20, device=DEV), saved, flat_grads=grads)
    assert ei.value.status == -2
    torch.cuda.synchronize()
    assert bool((grads == 3.0).all())
    # sizes depend on the mode: after the workspace is bound the setter answers FV_ERR_STATE, for a spec and for NULL alike
    assert eng._ws is not None
    assert rc(bins=32) == -2 and L.fv_head_set_bins(eng.h, None, None, None) == -2
    assert eng.head_bins["bins"] == 16
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the policy (synthetic:tiny:77)
NB, RNG = 32, (-2.0, 2.0)


def _policy(K=2, n_steps=1, seed=31, model="tiny:77", hd=(48, 64), sigma=0.0, decode="argmax", bins=NB, rng=RNG, **kw):
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{model}", hidden_dim=hd[0], fusion_dim=hd[1], dropout=0.0), chunk_size=K, n_action_steps=n_steps,
                         action_head="bins", action_bins=bins, action_bins_range=rng, action_bins_sigma=sigma, action_bins_decode=decode, **kw).to(DEV)


def _batch(B, K, A=14, seed=5, pads=None):
    g = torch.Generator().manual_seed(seed)
    pad = torch.zeros(B, K, dtype=torch.bool)
    for b, k in enumerate(pads if pads is not None else [(b + 1) % (K + 1) for b in range(B)]):
        if k:
            pad[b, K - k:] = True
    return {"images": torch.rand(B, 3, 72, 96, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, K, A, generator=g).clamp(-1.9, 1.9),
            "action_is_pad": pad, "tasks": ["stack the red block", "open drawer", "x", "push"][:B]}


def _dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _close(*pols):
    for p in pols:
        p.model.backbone.engine().close()


@pytest.mark.parametrize("sigma", [0.0, 0.75])
def test_training_drives_the_loss_down_and_the_accuracy_up(sigma):
    K = 2
    pol = _policy(K, sigma=sigma)
    pol.train()
    batch = _dev(_batch(4, K, pads=[0, 1, 0, 2]))
    prep = pol.prepare_batch(batch)
    outs = []
    for _ in range(100):
        o = pol.fused_train_step(prepared=prep, lr=5e-3, weight_decay=0.0, max_grad_norm=1.0)
        outs.append((float(o["loss"]), float(o["accuracy"]), float(o["mse"])))
    torch.cuda.synchronize()
    print(f"[bins training sigma={sigma}] loss {outs[0][0]:.4f} -> {outs[-1][0]:.4f}, accuracy {outs[0][1]:.3f} -> {outs[-1][1]:.3f}, decoded mse {outs[0][2]:.4f} -> {outs[-1][2]:.4f}")
    assert o["actions"].shape == (4, K, 14)
    # an untrained head starts near log(Nb) x the valid fraction 5 / 8 with about one hit in Nb; a hundred steps on one batch of 70 valid elements must at least
    # halve the loss and name the right bin for half of them
    assert outs[0][0] > 0.5 * np.log(NB) * 5 / 8 and outs[0][1] <= 0.25 and outs[-1][0] < 0.5 * outs[0][0]
    assert outs[-1][1] >= 0.5 and outs[-1][2] < outs[0][2]
    # compute_loss: the same loss kernel through autograd's surface; the accuracy rides in last_loss_metrics
    out = pol.compute_loss(batch)
    assert set(out) == {"loss", "mse", "accuracy"} and pol.last_loss_metrics.shape == (3,) and float(pol.last_loss_metrics[1]) == 5 / 8
    out["loss"].backward()
    assert tuple(pol.model.action_head.weight.grad.shape) == (K * 14 * NB, 64) and float(pol.model.action_head.weight.grad.abs().max()) > 0
    # the distributions: (B, K, A, Nb), rows sum to 1, their argmax is what predict decodes
    pol.eval()
    probs = pol.action_bin_probs(batch)
    assert probs.shape == (4, K, 14, NB) and float((probs.sum(-1) - 1).abs().max()) <= 1e-5
    with torch.no_grad():
        pred = pol(batch["images"], batch["states"], batch["tasks"])
    w = (RNG[1] - RNG[0]) / NB
    top2 = probs.topk(2, dim=-1).values
    clear = top2[..., 0] > top2[..., 1]                                       # (two logits a rounding apart can share one fp32 probability)
    assert pred.shape == (4, K, 14) and float(clear.float().mean()) >= 0.9
    assert torch.equal(pred[clear], (RNG[0] + (probs.argmax(-1).float() + 0.5) * w)[clear])
    with pytest.raises(ValueError, match="autograd"):
        pol(batch["images"], batch["states"], batch["tasks"])
    _close(pol)


def test_select_action_returns_unnormalised_bin_centres_and_honours_the_queue():
    K = 4
    pol = _policy(K, n_steps=3)
    g = torch.Generator().manual_seed(9)
    std, mean = torch.rand(14, generator=g) + 0.5, torch.randn(14, generator=g)
    pol.model.backbone.set_io_normalization(state_mean=torch.zeros(14), state_std=torch.ones(14), action_mean=mean, action_std=std)
    img, st = torch.rand(3, 72, 96, generator=g), torch.randn(14, generator=g)
    dev = torch.device(DEV)
    chunk = pol.select_action_chunk(img, st, "stack the red block", dev)
    assert chunk.shape == (K, 14) and not pol.training
    w = (RNG[1] - RNG[0]) / NB
    centres = (RNG[0] + (torch.arange(NB).float() + 0.5) * w).to(DEV)
    norm = (chunk - mean.to(DEV)) / std.to(DEV)
    nearest = centres[(norm.unsqueeze(-1) - centres).abs().argmin(-1)]
    assert float((norm - nearest).abs().max()) <= 1e-5                        # centre * std + mean of some bin
    assert torch.allclose(chunk, nearest * std.to(DEV) + mean.to(DEV), rtol=1e-6, atol=1e-6)
    eng = pol.model.backbone.engine()
    count = {"head": 0}
    head_fn = eng.head_forward
    eng.head_forward = lambda *a, **k: (count.__setitem__("head", count["head"] + 1), head_fn(*a, **k))[1]
    pol.reset()
    got = [pol.select_action(img, st, "stack the red block", dev) for _ in range(7)]
    assert count["head"] == 3                                                 # 7 calls at n_action_steps = 3: three plans
    for i, a_ in enumerate(got):
        assert torch.equal(a_, chunk[i % 3]), i
    eng.head_forward = head_fn
    _close(pol)


def test_it_composes_with_temporal_ensembling():
    K = 3
    pol = _policy(K, decode="mean", temporal_ensemble_coeff=0.1)
    g = torch.Generator().manual_seed(3)
    dev = torch.device(DEV)
    obs = [(torch.rand(3, 72, 96, generator=g), torch.randn(14, generator=g)) for _ in range(4)]
    chunks = [pol.select_action_chunk(i, s, "push", dev).double().cpu() for i, s in obs]
    pol.reset()
    acts = [pol.select_action(i, s, "push", dev).double().cpu() for i, s in obs]
    wts = np.exp(-0.1 * np.arange(K))
    for t in range(4):                                                        # step t averages what chunks t - K + 1 .. t predicted for it, the oldest weighted most
        rows = [chunks[j][t - j] for j in range(max(0, t - K + 1), t + 1)]
        ww = wts[: len(rows)]
        want = sum(w_ * r for w_, r in zip(ww, rows)) / ww.sum()
        assert float((acts[t] - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), t
    _close(pol)


def _train_rig(model, seed, hd, B, T, da, nb, ranges):
    w = weights.init_backbone(model, seed=seed)
    eng = FastVLAEngine(model, state_dim=14, action_dim=da, hidden_dim=hd, fusion_dim=hd, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng.set_head_bins(nb, ranges, 0.75, "mean")
    eng.load_weights(w)
    eng.train_begin()
    tensors, total, _nbk = eng.train_layout()
    flat = torch.zeros(total, dtype=torch.float32, device=DEV)
    eng.train_export_params(flat)
    lc = qwen2.Qwen2Cfg(hidden=model.llm.hidden, layers=model.llm.layers, heads=model.llm.heads, kv_heads=model.llm.kv_heads, head_dim=model.llm.head_dim,
                        inter=model.llm.inter, vocab=model.llm.vocab, rope_theta=model.llm.rope_theta, rms_eps=model.llm.rms_eps)
    g = torch.Generator().manual_seed(seed + 1)
    hp = {k: (torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
          for k, s in head.head_shapes(lc.hidden, 14, da * nb, hd, hd).items()}
    for k, v in eng.head_views(flat).items():
        v.copy_(hp[k])
    return w, eng, flat, lc, hp, tensors


def test_backbone_training_matches_autograd(monkeypatch):
    """the small preset (the decoder the backbone-training tests run), K = 2, HL-Gauss targets, a ragged mask: one full fine-tuning step against autograd -- the oracle of test_gpu_train_unfrozen with its one
    `F.mse_loss(pred, targets)` swapped for the float64 bins loss of the (B, K A Nb) logits it is handed (the pattern and bars of
    test_backbone_training_with_chunks_matches_autograd): the loss, and through _check_grads every gradient the step writes, d_pooled's descendants included.
    The smooth target distribution keeps the loss differentiable in the targets' neighbourhood: no element hangs on the bf16 backbone's last bits."""
    from test_gpu_train_unfrozen import GRAD_TOL, _check_grads, _inputs as _tu_inputs
    model = arch.preset("small")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, T, K, A, hd, nb = 3, 16, 2, 5, 64, 16
    da = K * A
    ranges = _ranges(A, nb)
    table = bins_table(ranges, nb, da)
    w, eng, flat, lc, hp, tensors = _train_rig(model, 41, hd, B, T, da, nb, ranges)
    assert {t["name"]: (t["rows"], t["cols"]) for t in tensors}["action_head.weight"] == (da * nb, hd)
    tower_out, ids, mask, states, _ = _tu_inputs(model, B, T, 42)
    pad = ragged_pad(B, K, seed=1)
    padt = torch.from_numpy(pad)
    eng.set_head_loss("mse", 1.0, K)
    targets = make_targets(B, K, A, table, nb, seed=43).view(B, da)
    ws = eng.train_workspace(B, T)
    fg = torch.zeros_like(flat)
    monkeypatch.setattr(F, "mse_loss", lambda pred, tgt: torch_bins_loss(pred.double().view(B, K, A, nb), tgt.view(B, K, A), table, padt, 0.75).to(pred.dtype))
    act, loss, grads = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, flat_grads=fg, pad=pad)
    met = eng.head_loss_metrics().cpu()
    torch.cuda.synchronize()
    ref = train_unfrozen.forward_backward(w, hp, tower_out.float(), ids, mask, states, targets, lc)
    rl = abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    dec = bins_ref(ref["pred"].double().numpy().reshape(B, K, A, nb), targets.numpy().reshape(B, K, A), table, pad, 0.75, "mean")
    ra = rel_l2(act.cpu().view(B, K, A)[~padt], torch.from_numpy(dec["decoded"])[~padt])
    worst = _check_grads(eng, grads, ref, tol=GRAD_TOL)
    print(f"[bins unfrozen small K={K} Nb={nb}] decoded actions rel_l2={ra:.2e} loss rel={rl:.2e} worst gradient: {worst[0]} {worst[1]:.2e}; metrics {met.tolist()}")
    assert act.shape == (B, da) and ra <= 1e-3 and rl <= 1e-3
    assert float(met[1]) == float(np.float32((~pad).sum() * A) / np.float32(B * da))
    eng.close()


def test_guard_delta_passes_through_the_bins_backward():
    """a bound guard at delta = 2^-2 over the static 2^12 against no guard and a static 2^10: the WHOLE gradient buffer bit for bit -- the delta multiply covers
    all Nb times wider dL/dlogits"""
    from fastvla_hip import StepGuard

    def make():
        torch.manual_seed(31)
        cfg = FastVLAConfig(vlm_model_name="synthetic:small:41", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)      # (test_gpu_step_guard.py's full_decoder rig)
        pol = FastVLAPolicy(cfg, chunk_size=2, action_head="bins", action_bins=NB, action_bins_range=RNG, action_bins_sigma=0.75).to(DEV)
        pol.train()
        pol.enable_backbone_training()
        return pol

    a, b = make(), make()
    ea, eb = a._unfrozen.eng, b._unfrozen.eng
    guard = StepGuard(ea, init_delta_log2=-2, min_delta_log2=-12, max_delta_log2=12)
    ea.train_set_step_guard(guard)
    eb.train_set_options(loss_scale_log2=10, keep=True)
    batch = _dev(_batch(2, 2, pads=[0, 1]))
    batch["images"] = torch.rand(2, 3, 96, 128, generator=torch.Generator().manual_seed(6)).to(DEV)
    kw = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    oa, ob = a.fused_train_step(batch, **kw), b.fused_train_step(batch, **kw)
    torch.cuda.synchronize()
    assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(oa["accuracy"], ob["accuracy"]) and torch.equal(oa["actions"], ob["actions"])
    ga, gb = a._unfrozen.g, b._unfrozen.g
    assert bool(torch.isfinite(ga).all()) and float(ga.abs().max()) > 0.0
    hv = ea.head_views(ga[: ea.head_numel()])["action_head.weight"]
    assert tuple(hv.shape) == (2 * 14 * NB, 64) and int((hv != 0).sum()) > hv.numel() // 4
    diff = int((ga.view(torch.int32) != gb.view(torch.int32)).sum())
    print(f"[bins step guard delta passthrough] {diff} of {ga.numel()} gradient elements differ")
    assert diff == 0
    ea.train_set_step_guard(None)
    guard.close()
    _close(a, b)


def test_checkpoint_round_trip_trainer_resume_and_cross_type_load(tmp_path):
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils import load_policy_from_checkpoint
    from vla_fastvlm.utils.checkpoint import save_policy_checkpoint
    K = 2
    per_dim = [(-2.0, 2.0), (-1.0, 3.0)] * 7
    pol = _policy(K, n_steps=2, seed=51, sigma=0.75, decode="mean", rng=per_dim)
    g = torch.Generator().manual_seed(9)
    img, st = torch.rand(3, 72, 96, generator=g), torch.randn(14, generator=g)
    chunk = pol.select_action_chunk(img, st, "open drawer", torch.device(DEV))
    d = save_policy_checkpoint(pol, tmp_path / "ck")
    ex = json.loads((d / "hip_extras.json").read_text())
    assert ex["action_head"] == {"type": "bins", "bins": NB, "range": [list(p) for p in per_dim], "sigma": 0.75, "decode": "mean"}
    assert ex["action_chunk"] == {"chunk_size": K, "n_action_steps": 2, "loss": "mse", "beta": 1.0}
    again = load_policy_from_checkpoint(str(d)).to(DEV)
    assert again.action_head == "bins" and again.model.bins == pol.model.bins and again.n_action_steps == 2
    assert torch.equal(again.select_action_chunk(img, st, "open drawer", torch.device(DEV)), chunk)
    _close(pol, again)

    # Trainer: two steps + resume + one step == three steps, bit for bit
    data = [_batch(2, K, seed=s) for s in (1, 2, 3)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1000, eval_steps=1000, seed=1)
    mk = lambda seed: _policy(K, seed=seed, sigma=0.75, decode="mean", rng=per_dim)      # noqa: E731
    a = mk(51)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=3, **tkw)).fit()
    b = mk(51)
    tb = Trainer(b, data[:2], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=2, max_steps=3, **tkw))
    tb.num_training_steps = 3
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-2"
    assert json.loads((ck / "hip_extras.json").read_text())["action_head"]["type"] == "bins"
    c = mk(99)      # another initialisation: everything comes from the checkpoint
    tc = Trainer(c, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    tc.num_training_steps = 3
    tc.fit()
    torch.cuda.synchronize()
    assert tc.update_step == 3 and c._opt_state["step"] == 3
    assert torch.equal(a.model._flat, c.model._flat) and torch.equal(a._opt_state["m"], c._opt_state["m"]) and torch.equal(a._opt_state["v"], c._opt_state["v"])
    # across head types: named, with action_head.weight's two shapes
    torch.manual_seed(51)
    plain = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K).to(DEV)
    with pytest.raises(ValueError) as ei:
        Trainer(plain, data, None, TrainingConfig(output_dir=str(tmp_path / "w"), max_steps=1, resume_from=str(ck), **tkw)).fit()
    assert "action_head.weight" in str(ei.value) and str((K * 14 * NB, 64)) in str(ei.value)
    assert str((K * 14, 64)) in str(ei.value)
    _close(a, b, c)
