"""-m gpu: the flow-matching action head -- the noising kernel (explicit inputs and its own draws), the head step in flow mode against float64 autograd, the
Euler sampler against the float64 reference and against the naive composition it replaces, the off switch, and the bimodal toy that is the point of it all.

Bars.  x_t, u: 1 ulp of the float64 formula rounded to fp32.  phi: SINCOS_ULP ulps of the float64 sin / cos of the fp32-rounded argument (see there).
Normals: flow_util.draw_normals' per-element bound.  Head step: test_gpu_action_chunk.test_head_step_matches_float64_autograd's measure and bars, unchanged
(the same kernels with a wider fusion.0).  Sampler: worst row against the RMS row norm, at most 4 x the distance of the fp32 CPU emulation from float64 for
the same case (the factor covers another summation order; tests/test_flow_host.py keeps that distance below 1e-4 for every case used here)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_util as fu  # noqa: E402
from chunk_loss_util import ragged_pad, torch_loss_ref  # noqa: E402
from gpu_util import DEV  # noqa: E402
from fastvla_hip import HEAD_KEYS, FastVLAEngine, _lib, arch  # noqa: E402

# sinf / cosf.  The HIP programming guide's math-API accuracy table is not part of the ROCm installation's documentation tree, so no bound can be cited from
# it here; the device library implements the OpenCL C functions, whose full profile allows sin / cos 4 ulp.  The bar is what an implementation that REDUCES
# THE ARGUMENT PROPERLY owes (the argument reaches ~1600 rad here, which is why the kernel calls sinf / cosf and not the fast intrinsics): the reduced
# argument r in [-pi/4, pi/4] rounded to fp32 moves sin r / cos r by at most half an ulp (|r cot r| <= 1, |r tan r| < 1), the polynomial and its evaluation
# in fp32 at most one ulp, the final rounding half an ulp: 2 ulp.  A reduction that loses bits at 1600 rad would show as hundreds of ulp.  The measured worst
# case is printed beside the bar.
SINCOS_ULP = 2.0


def _engine(name, B, flow=True, time_dist="uniform"):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=ds, action_dim=K * A, hidden_dim=hid, fusion_dim=fus, max_batch=max(B, 1))
    if flow:
        eng.set_head_flow(E, time_dist=time_dist)
    return eng


def _flat(eng, p):
    flat = torch.zeros(eng.head_numel(), device=DEV)
    for k, v in eng.head_views(flat).items():
        v.copy_(p[k])
    return flat


def _cat_view(eng, saved, B):
    """the (B, cw) cat matrix inside `saved`, found without knowing the layout: the head forward copies `pooled` into its first columns"""
    feat, cw = eng.head_dims["feat"], eng.head_cat_width()
    probe = torch.arange(1, B * feat + 1, dtype=torch.float32, device=DEV).view(B, feat) + 0.5
    flat = torch.zeros(eng.head_numel(), device=DEV)
    eng.head_forward(flat, probe, torch.zeros(B, eng.head_dims["ds"], device=DEV), saved=saved)
    torch.cuda.synchronize()
    off = int((saved == probe[0, 0]).nonzero()[0])
    cat = saved[off:off + B * cw].view(B, cw)
    assert torch.equal(cat[:, :feat], probe)
    return off, cat


# ------------------------------------------------------------------------------------------------------------------ 1. prepare, explicit noise and t
@pytest.mark.parametrize("B", [1, 9, 67])
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_prepare_with_explicit_noise_and_t(name, B):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    eng = _engine(name, B)
    g = torch.Generator().manual_seed(5 + B)
    a, eps, t = torch.randn(B, da, generator=g), torch.randn(B, da, generator=g), torch.rand(B, generator=g)
    t[0] = 1.0
    if B > 1:
        t[1] = 0.0
    if B > 2:
        eps[2] = -a[2] * 3                        # t eps and (1 - t) a cancel at t = 1 / 4
        t[2] = 0.25
    saved = eng.head_saved(B)
    off, cat = _cat_view(eng, saved, B)
    saved.fill_(float("nan"))
    before = saved.clone()
    u = eng.head_flow_prepare(a, saved, noise=eps, t=t)
    torch.cuda.synchronize()
    xo = feat + hid
    x_ref, u_ref = fu.noising_ref(a.numpy(), eps.numpy(), t.numpy())
    x_got, phi_got = cat[:, xo:xo + da].cpu().double().numpy(), cat[:, xo + da:].cpu().double().numpy()
    ex = np.abs(x_got - x_ref.astype(np.float32).astype(np.float64)) / fu.ulp32(x_ref)
    eu = np.abs(u.cpu().double().numpy() - u_ref.astype(np.float32).astype(np.float64)) / fu.ulp32(u_ref)
    phi_ref = fu.phi_ref(t.numpy(), fu.flow_freqs(E))
    ep = np.abs(phi_got - phi_ref) / fu.ulp32(phi_ref)
    print(f"[flow prepare {name} B={B}] worst error in ulp: x_t {ex.max():.2f} u {eu.max():.2f} phi {ep.max():.2f} (bar {SINCOS_ULP}); largest argument "
          f"{float(fu.phi_args(t.numpy(), fu.flow_freqs(E)).max()):.1f} rad")
    assert ex.max() <= 1.0 and eu.max() <= 1.0
    assert ep.max() <= SINCOS_ULP
    # nothing but the two new column blocks of cat was written
    mask = torch.ones_like(saved, dtype=torch.bool)
    mask.view(-1)[off:off + B * eng.head_cat_width()].view(B, -1)[:, xo:] = False
    assert bool(torch.isnan(saved[mask]).all()) and torch.equal(torch.isnan(saved), torch.isnan(before) & mask)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. prepare, internal draws
def test_prepare_draws_match_the_philox_reference():
    name, B, seed, offset = "awkward", 67, 0x1234_5678_9ABC, 77
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    eng = _engine(name, B)
    xo = feat + hid

    def run(Bc, off_, noise=None, targets=None):
        saved = eng.head_saved(Bc)
        _, cat = _cat_view(eng, saved, Bc)
        u = eng.head_flow_prepare(torch.zeros(Bc, da) if targets is None else targets, saved, seed=seed, offset=off_, noise=noise)
        torch.cuda.synchronize()
        return cat[:, xo:].clone().cpu(), u.cpu()

    # the uniform t, bit for bit: with a = 0 and eps = 1, x_t = t exactly
    xt, _ = run(B, offset, noise=torch.ones(B, da))
    t_ref = fu.draw_t_uniform(B, seed, offset)
    assert np.array_equal(xt[:, 0].numpy(), t_ref) and bool((xt[:, :da] == xt[:, :1]).all())
    # the normals: with a = 0, u = eps
    xt67, u67 = run(B, offset)
    n_ref, bar = fu.draw_normals(B, da, seed, offset)
    err = np.abs(u67.double().numpy() - n_ref)
    print(f"[flow draws] worst normal error / bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}; sample mean {float(u67.mean()):+.3f} std {float(u67.std()):.3f}")
    assert bool((err <= bar).all())
    # a row's draws do not depend on B; another offset changes every row
    xt3, u3 = run(3, offset)
    assert torch.equal(xt3, xt67[:3]) and torch.equal(u3, u67[:3])
    xto, uo = run(B, offset + 1)
    assert bool((uo != u67).any(dim=1).all()) and bool((xto[:, da:] != xt67[:, da:]).any(dim=1).all())
    eng.close()
    # logit-normal t against the float64 formula (expf and the division: a few ulp of a value in (0, 1))
    eng = _engine(name, B, time_dist="logit_normal")
    saved = eng.head_saved(B)
    _, cat = _cat_view(eng, saved, B)
    eng.head_flow_prepare(torch.zeros(B, da), saved, seed=seed, offset=offset, noise=torch.ones(B, da))
    torch.cuda.synchronize()
    t_ln = fu.draw_t_logit_normal(B, seed, offset, 0.0, 1.0)
    assert float(np.abs(cat[:, xo].cpu().double().numpy() - t_ln).max()) <= 1e-6
    eng.close()


def test_dropout_mask_is_unchanged_by_flow_mode():
    """the dropout stream of a (seed, offset) is the same stream with flow mode on: the keep pattern of a regression head and of a flow head agree"""
    name, B, seed, offset, p_drop = "awkward", 9, 99, 5, 0.5
    case = fu.sampler_case(name, B)
    fus, da = fu.DIMS[name][3], fu.DIMS[name][4] * fu.DIMS[name][5]
    masks = []
    for flow in (False, True):
        eng = _engine(name, B, flow=flow)
        saved = eng.head_saved(B)
        flat = torch.randn(eng.head_numel(), generator=torch.Generator().manual_seed(1)).to(DEV) * 0.1
        if flow:
            eng.head_flow_prepare(torch.zeros(B, da), saved, seed=seed, offset=offset)
        eng.head_forward(flat, case["pooled"].to(DEV), case["states"].to(DEV), training=True, dropout_p=p_drop, seed=seed, offset=offset, saved=saved)
        torch.cuda.synchronize()
        # the mask block: B * fus values that are exactly 0 or 1 / (1 - p), the only such run in `saved`
        keep = ((saved == 0) | (saved == 1.0 / (1.0 - p_drop))).cpu().numpy().astype(np.int8)
        runs = np.flatnonzero(np.convolve(keep, np.ones(B * fus, dtype=np.int64), "valid") == B * fus)
        assert len(runs) >= 1                   # (dropped elements at the end of the block before it lengthen the run to the front: the last start is the block's)
        masks.append(saved[int(runs[-1]):int(runs[-1]) + B * fus].clone().cpu())
        eng.close()
    assert torch.equal(masks[0], masks[1]) and 0.2 < float((masks[0] == 0).float().mean()) < 0.8


# ------------------------------------------------------------------------------------------------------------------ 3. the head step against float64 autograd
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_flow_head_step_matches_float64_autograd(name, B, kind):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    p = fu.flow_head_params(fu.flow_head_shapes(feat, ds, da, hid, fus, E), 7, scale=0.2 if name == "awkward" else 0.05)
    g = torch.Generator().manual_seed(8 + B)
    pooled, states = torch.randn(B, feat, generator=g), torch.randn(B, ds, generator=g)
    a, eps, t = torch.randn(B, da, generator=g), torch.randn(B, da, generator=g), torch.rand(B, generator=g)
    pad = ragged_pad(B, K, seed=1) if B * K > 1 else np.zeros((B, K), dtype=bool)
    eng = _engine(name, B)
    eng.set_head_loss(kind, 1.0, K)
    flat = _flat(eng, p)
    saved = eng.head_saved(B)
    u = eng.head_flow_prepare(a, saved, noise=eps, t=t)
    v, _ = eng.head_forward(flat, pooled.to(DEV), states.to(DEV), saved=saved, normalized_actions=True)
    loss, grads = eng.head_backward(flat, v, u, saved, pad=pad)
    torch.cuda.synchronize()
    # float64: the noising formula, phi of the fp32-rounded argument (the device's definition of the embedding), the same network, the same loss
    x_ref, u_ref = fu.noising_ref(a.numpy(), eps.numpy(), t.numpy())
    p64 = {k: w.double().requires_grad_(True) for k, w in p.items()}
    pooled64 = pooled.double().requires_grad_(True)
    pred = fu.velocity(p64, pooled64, states.double(), torch.from_numpy(x_ref), torch.from_numpy(fu.phi_ref(t.numpy(), fu.flow_freqs(E))))
    ref = torch_loss_ref(pred.view(B, K, A), torch.from_numpy(u_ref).view(B, K, A), torch.from_numpy(pad), kind, 1.0)
    ref.backward()
    np.testing.assert_allclose(v.cpu().numpy(), pred.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    gv = eng.head_views(grads)
    worst = 0.0
    for k in HEAD_KEYS:
        r = p64[k].grad
        bar = 2e-5 * max(1e-3, float(r.abs().max()))
        err = float((gv[k].cpu().double() - r).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (k, err, bar)
    # d_pooled, the gradient an unfrozen backbone continues from: the first feat columns of the (now wider) dcat.  The test-only entry point runs the same
    # launch_head_backward and hands it out; its 12 gradients are the product call's, bit for bit
    from gpu_util import lib, stream
    G2, dp = torch.full_like(grads, float("nan")), torch.full((B, feat), float("nan"), device=DEV)
    loss2, met, scr = torch.zeros(1, device=DEV), torch.zeros(4, device=DEV), torch.zeros(B * da + 2 * B * max(eng.head_cat_width(), fus) + 64 + 768, device=DEV)
    padd = torch.from_numpy(pad).to(DEV, torch.uint8).contiguous()
    _lib.check(lib().fv_op_head_loss_backward(feat, ds, da, hid, fus, E, flat.data_ptr(), v.data_ptr(), u.data_ptr(), padd.data_ptr(), _lib.LOSS_KINDS[kind], 1.0, K, B,
                                              saved.data_ptr(), loss2.data_ptr(), met.data_ptr(), G2.data_ptr(), scr.data_ptr(), scr.numel(), dp.data_ptr(), stream()),
               "fv_op_head_loss_backward")
    torch.cuda.synchronize()
    assert all(torch.equal(t2, gv[k]) for k, t2 in eng.head_views(G2).items()) and torch.equal(loss2, loss)      # (views: the flat buffer has alignment gaps)
    r = pooled64.grad
    bar = 2e-5 * max(1e-3, float(r.abs().max()))
    err = float((dp.cpu().double() - r).abs().max())
    assert err <= bar, ("d_pooled", err, bar)
    print(f"[flow head step {name} B={B} {kind}] worst gradient error / bar {worst:.3f}; d_pooled {err / bar:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the sampler against the float64 Euler reference
def _set_io(eng, st, on):
    if on:
        eng.set_io_norm(st["state_mean"], st["state_std"], st["action_mean"], st["action_std"])
    else:
        eng.set_io_norm()


@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_sampler_matches_float64_euler(name, B):
    case = fu.sampler_case(name, B)
    eng = _engine(name, B)
    flat = _flat(eng, case["p"])
    worst = 0.0
    for io in (False, True):
        _set_io(eng, case["stats"], io)
        for N in fu.SAMPLER_STEPS:
            got = eng.head_flow_sample(flat, case["pooled"].to(DEV), case["states"].to(DEV), steps=N, noise=case["noise"])
            torch.cuda.synchronize()
            ref, emu = fu.sampler_refs(case, N, io)
            err = fu.worst_row_vs_rms(got.cpu(), ref)
            worst = max(worst, err / (4 * emu))
            print(f"[flow sampler {name} B={B} N={N} io={int(io)}] error {err:.3e}, fp32 emulation {emu:.3e}, error / bar {err / (4 * emu):.3f}")
            assert bool(torch.isfinite(got).all()) and err <= 4 * emu
    print(f"[flow sampler {name} B={B}] worst error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. hoisting cross-check
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 3)])
def test_sampler_equals_the_naive_composition_and_repeats_its_bits(name, B):
    """N x (x and phi(t_i) written into `saved`, fv_head_forward, host Euler step): the conditioning recomputed every step.  x and phi(t_i) get there through
    fv_head_flow_prepare(targets = x, noise = x, t = t_i): t x + (1 - t) x is x exactly after the kernel's one rounding from double."""
    N = 10
    case = fu.sampler_case(name, B)
    da = fu.DIMS[name][4] * fu.DIMS[name][5]
    eng = _engine(name, B)
    flat = _flat(eng, case["p"])
    pooled, states = case["pooled"].to(DEV), case["states"].to(DEV)
    got = eng.head_flow_sample(flat, pooled, states, steps=N, noise=case["noise"])
    again = eng.head_flow_sample(flat, pooled, states, steps=N, noise=case["noise"])
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    drawn = [eng.head_flow_sample(flat, pooled, states, steps=N, seed=3, offset=4).clone() for _ in range(2)]
    assert torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[0], got)
    saved, x = eng.head_saved(B), case["noise"].to(DEV).clone()
    ts, dt = fu.step_times(N), float(np.float32(-1.0 / N))
    for i in range(N):
        eng.head_flow_prepare(x, saved, noise=x, t=torch.full((B,), float(ts[i])))
        v, _ = eng.head_forward(flat, pooled, states, saved=saved)
        x = x + dt * v
    torch.cuda.synchronize()
    _, emu = fu.sampler_refs(case, N, False)
    err = fu.worst_row_vs_rms(got.cpu(), x.cpu())
    print(f"[flow hoisting {name} B={B}] sampler vs naive composition {err:.3e} (bar {4 * emu:.3e})")
    assert err <= 4 * emu
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. off means off
def test_off_means_off_and_the_setter_checks():
    name, B = "awkward", 5
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    fresh, seen = _engine(name, B, flow=False), _engine(name, B, flow=False)
    L = seen.lib
    n0 = seen.head_numel()
    # every bad specification: FV_ERR_ARG, nothing changed
    bad = [(0, 4e-3, 4.0, 0, 0.0, 1.0), (-2, 4e-3, 4.0, 0, 0.0, 1.0), (7, 4e-3, 4.0, 0, 0.0, 1.0), (6, 0.0, 4.0, 0, 0.0, 1.0), (6, -1.0, 4.0, 0, 0.0, 1.0),
           (6, 4.0, 4e-3, 0, 0.0, 1.0), (6, 4.0, 4.0, 0, 0.0, 1.0), (6, float("nan"), 4.0, 0, 0.0, 1.0), (6, 4e-3, float("inf"), 0, 0.0, 1.0),
           (6, 4e-3, 4.0, 2, 0.0, 1.0), (6, 4e-3, 4.0, -1, 0.0, 1.0), (6, 4e-3, 4.0, 1, float("nan"), 1.0), (6, 4e-3, 4.0, 1, 0.0, float("inf"))]
    for spec in bad:
        assert L.fv_head_set_flow(seen.h, C.byref(_lib.HeadFlowSpec(*spec))) == -1, spec
    assert L.fv_head_set_flow(None, None) == -1
    offs = (C.c_int64 * 13)()
    assert L.fv_head_layout(seen.h, C.byref(offs)) == 0 and list(offs) == fresh.head_offsets
    # flow entry points on a regression head: FV_ERR_STATE
    buf = torch.full((4096,), float("nan"), device=DEV)
    assert L.fv_head_flow_prepare(seen.h, buf.data_ptr(), 1, 0, 0, None, None, buf.data_ptr(), buf.data_ptr(), None) == -2
    assert L.fv_head_flow_sample(seen.h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 10, None, 0, 0, buf.data_ptr(), None) == -2
    # on, then off again: the layout, the saved size and the bits of a step are those of a handle that never saw the call
    seen.set_head_flow(E)
    assert seen.head_numel() == n0 + fus * (da + E) and seen.head_saved(B).numel() > fresh.head_saved(B).numel()
    # bad sampler / prepare arguments in flow mode: their code, and nothing enqueued (every byte of the buffers they were handed keeps its NaN)
    flat_f = torch.zeros(seen.head_numel(), device=DEV)
    pooled, states = torch.zeros(B, feat, device=DEV), torch.zeros(B, ds, device=DEV)
    out = torch.full((B, da), float("nan"), device=DEV)
    sv = seen.head_saved(B).fill_(float("nan"))
    args = (flat_f.data_ptr(), pooled.data_ptr(), states.data_ptr())
    assert L.fv_head_flow_sample(seen.h, *args, B, 10, None, 0, 0, out.data_ptr(), None) == -2            # no workspace bound yet
    seen.ensure_workspace(B, 1, False)
    assert L.fv_head_flow_sample(seen.h, *args, B, 0, None, 0, 0, out.data_ptr(), None) == -1
    assert L.fv_head_flow_sample(seen.h, *args, B, -3, None, 0, 0, out.data_ptr(), None) == -1
    assert L.fv_head_flow_sample(seen.h, *args, B + 1, 10, None, 0, 0, out.data_ptr(), None) == -1           # B > max_batch
    assert L.fv_head_flow_sample(seen.h, *args, 0, 10, None, 0, 0, out.data_ptr(), None) == -1
    assert L.fv_head_flow_sample(seen.h, None, args[1], args[2], B, 10, None, 0, 0, out.data_ptr(), None) == -1
    assert L.fv_head_flow_sample(seen.h, *args, B, 10, None, 0, 0, None, None) == -1
    assert L.fv_head_flow_prepare(seen.h, None, B, 0, 0, None, None, sv.data_ptr(), out.data_ptr(), None) == -1
    assert L.fv_head_flow_prepare(seen.h, out.data_ptr(), 0, 0, 0, None, None, sv.data_ptr(), out.data_ptr(), None) == -1
    assert L.fv_head_flow_prepare(seen.h, out.data_ptr(), B, 0, 0, None, None, None, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(sv).all())
    # the workspace is bound now: sizes depend on the mode, so the setter refuses, both ways
    assert L.fv_head_set_flow(seen.h, None) == -2 and L.fv_head_set_flow(seen.h, C.byref(_lib.HeadFlowSpec(8, 4e-3, 4.0, 0, 0.0, 1.0))) == -2
    assert b"fv_bind_workspace" in L.fv_last_error(seen.h)
    seen.close()
    seen = _engine(name, B, flow=False)
    seen.set_head_flow(E)
    seen.set_head_flow(None)
    assert seen.head_offsets == fresh.head_offsets and seen.head_saved(B).numel() == fresh.head_saved(B).numel()
    p = fu.flow_head_params({k: s for k, s in fu.flow_head_shapes(feat, ds, da, hid, fus, 0).items()}, 3)
    p["fusion.0.weight"] = p["fusion.0.weight"][:, :feat + hid].contiguous()
    g = torch.Generator().manual_seed(4)
    pooled, states, tgt = torch.randn(B, feat, generator=g), torch.randn(B, ds, generator=g), torch.randn(B, da, generator=g)
    outs = []
    for eng in (fresh, seen):
        flat = _flat(eng, p)
        act, saved = eng.head_forward(flat, pooled.to(DEV), states.to(DEV), training=True, dropout_p=0.1, seed=7, offset=3)
        loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved, dropout_p=0.1)
        torch.cuda.synchronize()
        outs.append((act.clone(), loss.clone(), grads.clone()))      # (`saved` itself has alignment gaps that nobody writes)
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    fresh.close(), seen.close()


# ------------------------------------------------------------------------------------------------------------------ 8. the bimodal toy
def _train_head(eng, flat, pooled, states, targets, steps, lr, flow, seed=11):
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    B = pooled.shape[0]
    saved = eng.head_saved(B)
    for it in range(1, steps + 1):
        if flow:
            tgt = eng.head_flow_prepare(targets, saved, seed=seed, offset=it)
        else:
            tgt = targets
        out, _ = eng.head_forward(flat, pooled, states, saved=saved, normalized_actions=True)
        _, grads = eng.head_backward(flat, out, tgt, saved)
        eng.adamw_step(flat, grads, m, v, it, lr=lr, weight_decay=0.0, max_grad_norm=0.0)


def test_bimodal_toy_flow_keeps_both_modes_where_regression_averages_them():
    """a fixed observation, targets +1 or -1 (all dimensions jointly) with probability 1 / 2: the regression head learns their mean, 0; the flow head's samples
    land near +1 or near -1.  The recipe (fu.BIMODAL) is the one tests/test_flow_host.py runs on the torch reference with stricter thresholds."""
    r = fu.BIMODAL
    feat, ds, hid, fus, K, A, E = r["dims"]
    da, B = K * A, r["batch"]
    targets = fu.bimodal_targets(B, da, r["seed"]).to(DEV)
    pooled, states = fu.bimodal_observation(B, feat, ds)
    res = {}
    for flow in (True, False):
        m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                             arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
        eng = FastVLAEngine(m, state_dim=ds, action_dim=da, hidden_dim=hid, fusion_dim=fus, max_batch=256)
        if flow:
            eng.set_head_flow(E)
        flat = _flat(eng, fu.bimodal_init(feat, ds, da, hid, fus, E if flow else None, r["seed"]))
        _train_head(eng, flat, pooled.to(DEV), states.to(DEV), targets, r["steps"], r["lr"], flow)
        po, so = pooled[:1].expand(256, -1).contiguous().to(DEV), states[:1].expand(256, -1).contiguous().to(DEV)
        if flow:
            out = eng.head_flow_sample(flat, po, so, steps=10, seed=5, offset=1)
        else:
            out, _ = eng.head_forward(flat, po, so)
        torch.cuda.synchronize()
        res[flow] = fu.mode_stats(out.cpu())
        eng.close()
    print(f"[flow bimodal] flow: {res[True]}; regression: {res[False]}")
    assert res[True]["plus"] >= 0.25 and res[True]["minus"] >= 0.25 and res[True]["mean_abs"] >= 0.7
    assert res[False]["mean_abs"] <= 0.2


# ------------------------------------------------------------------------------------------------------------------ 7. the backbone routes
def _route_rig(model, seed, hd, B, T, da, E, toggle=False):
    from oracle import qwen2
    from fastvla_hip import weights
    w = weights.init_backbone(model, seed=seed)
    eng = FastVLAEngine(model, state_dim=14, action_dim=da, hidden_dim=hd, fusion_dim=hd, max_batch=B, max_text_tokens=T, llm_precision=1)
    if E:
        eng.set_head_flow(E)
    if toggle:
        eng.set_head_flow(6)
        eng.set_head_flow(None)
    eng.load_weights(w)
    eng.train_begin()
    _, total, _ = eng.train_layout()
    flat = torch.zeros(total, dtype=torch.float32, device=DEV)
    eng.train_export_params(flat)
    g = torch.Generator().manual_seed(seed + 1)
    shapes = fu.flow_head_shapes(model.llm.hidden, 14, da, hd, hd, E)
    if not E:
        shapes["fusion.0.weight"] = (hd, model.llm.hidden + hd)
    hp = {k: (torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
          for k, s in shapes.items()}
    for k, v in eng.head_views(flat).items():
        v.copy_(hp[k])
    return w, eng, flat


def test_backbone_routes_noise_like_the_head_only_route():
    """synthetic:small, K = 4, flow mode: one full fine-tuning step and one rank-16 projected LoRA step.  Their loss and 12 head gradients against the head-only
    route (fv_head_flow_prepare + fv_head_forward + fv_head_mse_backward) on the same (seed, offset, targets) and the pooled feature of an inference forward;
    bars of test_gpu_action_chunk.test_backbone_training_with_chunks_matches_autograd (loss 1e-3 relative, gradients rel_l2 2e-3: the inference forward and
    the training forward run the bf16 backbone through different kernels).  Then the same step WITHOUT flow on a handle that set flow and unset it: bitwise
    the step of a handle that never saw the call."""
    from gpu_util import rel_l2
    from oracle import fastvit_hd
    from test_gpu_lora import _random_adapters
    from test_gpu_train_unfrozen import GRAD_TOL, _inputs
    model = arch.preset("small")
    B, T, K, A, hd, E, rank, seed, offset = 3, 16, 4, 5, 64, 6, 16, 1234, 9
    da = K * A
    w, eng, flat = _route_rig(model, 41, hd, B, T, da, E)
    tower_out, ids, mask, states, _ = _inputs(model, B, T, 42)
    targets = torch.randn(B, da, generator=torch.Generator().manual_seed(43))
    eng.set_head_loss("mse", 1.0, K)
    ws = eng.train_workspace(B, T)
    fg = torch.zeros_like(flat)

    def head_only():
        with torch.no_grad():
            tok = fastvit_hd.projector_forward(w, tower_out.float()).to(DEV)
        pooled = eng.llm_pooled(ids, mask.sum(1), tok)
        hflat = flat[: eng.head_numel()].clone()
        saved = eng.head_saved(B)
        u = eng.head_flow_prepare(targets, saved, seed=seed, offset=offset)
        v, _ = eng.head_forward(hflat, pooled, states.to(DEV), saved=saved, normalized_actions=True)
        loss, grads = eng.head_backward(hflat, v, u, saved)
        torch.cuda.synchronize()
        return v.clone(), float(loss), {k: t.clone() for k, t in eng.head_views(grads).items()}

    def check(what, act, loss, grads_flat, ref):
        rv, rl, rg = ref
        got = eng.head_views((grads_flat / eng.train_loss_scale())[: eng.head_numel()])
        errs = sorted(((rel_l2(got[k].cpu(), rg[k].cpu()), k) for k in HEAD_KEYS), reverse=True)
        ra, el = rel_l2(act.cpu(), rv.cpu()), abs(float(loss) - rl) / rl
        print(f"[flow route {what}] velocity rel_l2={ra:.2e} loss rel={el:.2e}; worst head gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
        assert ra <= 1e-3 and el <= 1e-3
        for e, k in errs:
            assert e <= GRAD_TOL, (what, k, e)

    ref = head_only()
    act, loss, grads = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, seed=seed, offset=offset, flat_grads=fg)
    torch.cuda.synchronize()
    check("full", act, loss, grads, ref)
    act2, loss2, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, seed=seed, offset=offset + 1, flat_grads=fg.clone())
    torch.cuda.synchronize()
    assert not torch.equal(act2, act)                                           # another offset: another x_t
    # rank-16 LoRA, projected backward
    eng.train_lora_begin(rank, 2.0 * rank, None)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    eng.train_lora_commit(flat, lflat)
    ref = head_only()                                                           # (the inference forward now runs the adapted weights)
    actp, lossp, gp = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, seed=seed, offset=offset, flat_grads=fg)
    torch.cuda.synchronize()
    check("lora r=16", actp, lossp, gp, ref)
    eng.close()
    # off means off on the training route too
    outs = []
    for toggle in (False, True):
        _, e2, f2 = _route_rig(model, 41, hd, B, T, da, 0, toggle=toggle)
        e2.set_head_loss("mse", 1.0, K)
        a, l, g = e2.train_forward_backward(f2, tower_out.to(DEV), ids, mask.sum(1), states, targets, e2.train_workspace(B, T), training=False, seed=seed, offset=offset,
                                            flat_grads=torch.zeros_like(f2))
        torch.cuda.synchronize()
        outs.append((a.clone(), l.clone(), g.clone()))
        e2.close()
    assert all(torch.equal(x, y) for x, y in zip(*outs))


# ------------------------------------------------------------------------------------------------------------------ 9. surfaces
def _flow_policy(K=3, n_steps=1, seed=31, flow=True, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(seed)
    extra = dict(action_head="flow", flow_time_dim=6, flow_seed=77) if flow else dict(action_head="regression")
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K, n_action_steps=n_steps,
                         **extra, **kw).to(DEV)


def _batch(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    pad = torch.zeros(B, K, dtype=torch.bool)
    pad[0, K - 1:] = True
    return {"images": torch.rand(B, 3, 72, 96, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, K, 14, generator=g),
            "action_is_pad": pad, "tasks": ["stack the red block", "open drawer", "x", "push"][:B]}


def _dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def test_core_policy_surface_in_flow_mode(tmp_path, monkeypatch):
    import json
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils import load_policy_from_checkpoint
    from vla_fastvlm.utils.checkpoint import save_policy_checkpoint
    for k in ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_STEPS", "FASTVLA_FLOW_TIME_DIM", "FASTVLA_FLOW_TIME_DIST"):
        monkeypatch.delenv(k, raising=False)
    K, B = 3, 2
    pol = _flow_policy(K, n_steps=2)
    m = pol.model
    assert pol.action_head == "flow" and pol.flow_steps == 10 and m.fusion[0].weight.shape == (64, m.backbone.output_dim + 48 + K * 14 + 6)
    batch = _dev(_batch(B, K, 5))
    img, st, task = batch["images"][0], batch["states"][0], "open drawer"
    # select_action with the queue: one sampler call serves two steps
    a1, a2 = pol.select_action(img, st, task, DEV), pol.select_action(img, st, task, DEV)
    assert a1.shape == (14,) and bool(torch.isfinite(a1).all() and torch.isfinite(a2).all()) and m._flow_sample_calls == 1 and not torch.equal(a1, a2)
    pol.select_action(img, st, task, DEV)
    assert m._flow_sample_calls == 2
    pol.reset()
    # the chunk is the library's sampler on the policy's pooled feature with the policy's stream; flow_steps may change at any time
    eng = m._engine()
    with torch.no_grad():
        pooled = m.features(pol.processor.prepare_images(img.unsqueeze(0), DEV), pol.processor.prepare_tasks(task, batch_size=1), device=DEV)
        want = eng.head_flow_sample(m._flat, pooled, pol.processor.prepare_states(st.unsqueeze(0), DEV), steps=10, seed=m._flow_seed, offset=(1 << 62) + m._flow_sample_calls + 1)
    chunk = pol.select_action_chunk(img, st, task, DEV)
    assert chunk.shape == (K, 14) and torch.equal(chunk.reshape(1, -1), want)
    pol.flow_steps = 4
    assert not torch.equal(pol.select_action_chunk(img, st, task, DEV), chunk) and m.flow_steps == 4
    with pytest.raises(ValueError):
        pol.flow_steps = 0
    pol.flow_steps = 10
    # sampling is not differentiated
    pol.train()
    with pytest.raises(RuntimeError, match="not differentiated"):
        pol.forward(batch["images"], batch["states"], batch["tasks"])
    # the loss: differentiable w.r.t. the head in train mode; in eval mode a function of the evaluation batch index
    out = pol.compute_loss(batch)
    out["loss"].backward()
    assert all(p_.grad is not None and float(p_.grad.abs().max()) > 0 for p_ in m.head_parameters()) and float(out["loss"].detach()) > 0
    pol.eval()
    with torch.no_grad():
        e1 = [float(pol.compute_loss(b)["loss"]) for b in (batch, batch)]
    pol.eval()
    with torch.no_grad():
        e2 = [float(pol.compute_loss(b)["loss"]) for b in (batch, batch)]
    assert e1 == e2 and e1[0] != e1[1]
    # checkpoint round trip with the action_head record
    ck = save_policy_checkpoint(pol, tmp_path / "flow")
    rec = json.loads((ck / "hip_extras.json").read_text())["action_head"]
    assert rec == {"type": "flow", "steps": 10, "time_dim": 6, "min_period": 4e-3, "max_period": 4.0, "time_dist": "uniform", "dist_a": 0.0, "dist_b": 1.0, "seed": 77}
    back = load_policy_from_checkpoint(str(ck), DEV).to(DEV)
    assert back.action_head == "flow" and back.flow_steps == 10 and back.chunk_size == K and back.n_action_steps == 2
    back.model._flow_sample_calls = m._flow_sample_calls
    assert torch.equal(back.select_action_chunk(img, st, task, DEV), pol.select_action_chunk(img, st, task, DEV))
    # temporal ensembling works on the sampled chunk
    ens = _flow_policy(K, n_steps=1, temporal_ensemble_coeff=0.1)
    acts = [ens.select_action(img, st, task, DEV) for _ in range(3)]
    assert all(a.shape == (14,) and bool(torch.isfinite(a).all()) for a in acts) and ens.model._flow_sample_calls == 3
    # a regression checkpoint does not load into a flow policy, nor the reverse: both messages name fusion.0.weight's shapes and the setting
    reg = _flow_policy(K, n_steps=2, flow=False)
    reg.model.materialize(torch.device(DEV))
    assert "action_head" not in json.loads((save_policy_checkpoint(reg, tmp_path / "reg") / "hip_extras.json").read_text())
    for target, src in ((reg, tmp_path / "flow"), (pol, tmp_path / "reg")):
        tr = Trainer(target, [], None, TrainingConfig(output_dir=str(tmp_path / "x"), max_steps=1))
        with pytest.raises(ValueError, match=r"fusion\.0\.weight is \(64, \d+\) in the checkpoint and \(64, \d+\) in this policy.*action_head="):
            tr._load_checkpoint(str(src))
    # EMA covers the flow head's 12 tensors like any other head's
    pol.train()
    pol.enable_ema(decay=0.9)
    o = pol.fused_train_step(batch, lr=1e-3)
    torch.cuda.synchronize()
    assert o["actions"].shape == (B, K, 14) and pol.ema_shadow.numel() == m._flat.numel() and float(o["loss"]) > 0
    for p_ in (pol, back, ens, reg):
        p_.model.backbone.engine().close()


def test_resumed_trainer_continues_the_noise_stream(tmp_path, monkeypatch):
    """3 updates, save, resume in a fresh flow policy, 2 more == an uninterrupted 5-update run, bit for bit in the parameters and the moments: the noise of a
    train step is a function of (flow seed, optimiser step), both of which the checkpoint carries"""
    from vla_fastvlm.training import Trainer, TrainingConfig
    for k in ("FASTVLA_ACTION_HEAD", "FASTVLA_EMA_DECAY"):
        monkeypatch.delenv(k, raising=False)
    K = 3
    data = [_batch(4, K, s) for s in (31, 32, 33, 34, 35)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1, eval_steps=1000, seed=1)
    a = _flow_policy(K)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=5, **tkw)).fit()
    b = _flow_policy(K)
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=5, **tkw))
    tb.num_training_steps = 5
    tb.fit()
    c = _flow_policy(K, seed=99)
    c.model._flow_seed = 5          # (a fresh policy's own seed: the checkpoint's replaces it)
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=5, resume_from=str(tmp_path / "b" / "checkpoints" / "step-3"), **tkw))
    tc.num_training_steps = 5
    tc.fit()
    torch.cuda.synchronize()
    assert c._opt_state["step"] == 5 and c.model._flow_seed == 77
    assert torch.equal(c.model._flat, a.model._flat) and torch.equal(c._opt_state["m"], a._opt_state["m"]) and torch.equal(c._opt_state["v"], a._opt_state["v"])
    assert not torch.equal(b.model._flat, a.model._flat)
    for p_ in (a, b, c):
        p_.model.backbone.engine().close()


def test_lerobot_surface_in_flow_mode(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    K, A, B = 4, 5, 2
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}

    def cfg(n):
        return LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=n,
                        output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)

    monkeypatch.setenv("FASTVLA_ACTION_HEAD", "flow")          # the twin selects it; an argument beats the twin
    monkeypatch.setenv("FASTVLA_FLOW_TIME_DIM", "6")
    torch.manual_seed(3)
    assert LRPolicy(cfg(3), action_head="regression").model.flow is None
    pol = LRPolicy(cfg(3), flow_steps=5, flow_seed=11).to(DEV)
    assert pol.action_head == "flow" and pol.model.flow["time_dim"] == 6 and pol.model.flow_steps == 5
    g = torch.Generator().manual_seed(4)
    batch = {"observation.images.top": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(B, 6, generator=g).to(DEV), "task": ["a", "b"]}
    chunk = pol.predict_action_chunk(batch)
    assert chunk.shape == (B, K, A) and bool(torch.isfinite(chunk).all())
    acts = [pol.select_action(batch) for _ in range(4)]          # n_action_steps = 3: the fourth call samples again
    assert all(a.shape == (B, A) for a in acts) and pol.model._flow_sample_calls == 3
    pol.train()
    loss, info = pol.forward({**batch, ACTION: torch.randn(B, K, A, generator=g).to(DEV), "action_is_pad": torch.zeros(B, K, dtype=torch.bool)})
    loss.backward()
    assert float(loss.detach()) > 0 and all(p_.grad is not None and float(p_.grad.abs().max()) > 0 for p_ in pol.model.head_parameters())
    monkeypatch.delenv("FASTVLA_ACTION_HEAD")
    ens = LRPolicy(cfg(1), action_head="flow", temporal_ensemble_coeff=0.1).to(DEV)
    assert all(bool(torch.isfinite(ens.select_action(batch)).all()) for _ in range(3))
    pol.model.backbone.engine().close(), ens.model.backbone.engine().close()


def test_ema_scope_and_merge_lora_in_flow_mode(monkeypatch):
    """synthetic:small, K = 4, flow head, rank-16 LoRA, EMA on, three train steps.  Inside ema_weights() sampling and the evaluation loss use the AVERAGED
    weights -- they equal a second policy committed from the average -- and on exit the live buffer, the sampled chunk (same noise offset) and the loss are
    back bit for bit.  merge_lora() then folds the adapters into the master: the chunk sampled at the same offset and the loss stay within the 1e-5 that
    tests/test_gpu_lora.py / test_gpu_ema.py hold a merged model to against the adapted one."""
    from gpu_util import rel_l2
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    for k in ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER", "FASTVLA_ACTION_HEAD", "FASTVLA_LORA_RANK", "FASTVLA_LORA_DIRECT"):
        monkeypatch.delenv(k, raising=False)
    K, B = 4, 2

    def build(ema):
        torch.manual_seed(31)
        cfg = FastVLAConfig(vlm_model_name="synthetic:small:41", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
        pol = FastVLAPolicy(cfg, chunk_size=K, action_head="flow", flow_time_dim=6, flow_seed=77).to(DEV)
        pol.train()
        pol.enable_backbone_training(lora_rank=16, lora_alpha=32.0)
        if ema:
            pol.enable_ema(decay=0.9, warmup=True, update_after=1)
        return pol

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        return {"images": torch.rand(B, 3, 96, 128, generator=g).to(DEV), "states": torch.randn(B, 14, generator=g).to(DEV),
                "actions": torch.randn(B, K, 14, generator=g).to(DEV), "tasks": ["pick up the red cube", "open the drawer"]}

    def sample(pol, b):
        pol.eval()
        pol.model._flow_sample_calls = 0          # the same noise offset every time
        with torch.no_grad():
            out = pol(b["images"], b["states"], b["tasks"]).clone()
        torch.cuda.synchronize()
        return out

    def eval_loss(pol, b):
        pol.eval()                                # (restarts the evaluation batch index: the same noise every time)
        with torch.no_grad():
            return float(pol.compute_loss(b)["loss"])

    pol = build(True)
    for seed in (11, 12, 13):
        out = pol.fused_train_step(batch(seed), lr=2e-3, weight_decay=1e-2)
    torch.cuda.synchronize()
    assert out["actions"].shape == (B, K, 14) and float(out["loss"]) > 0 and pol._unfrozen.lora["rank"] == 16
    b = batch(21)
    live_s, live_l = sample(pol, b), eval_loss(pol, b)
    assert live_s.shape == (B, K, 14) and bool(torch.isfinite(live_s).all()) and torch.equal(sample(pol, b), live_s) and eval_loss(pol, b) == live_l
    live_buf, live_ptr = pol._ema_live().detach().clone(), pol._ema_live().data_ptr()
    ref = build(False)                            # the average, committed into a second policy
    ref._ema_live().copy_(pol.ema_shadow)
    ref._unfrozen.commit()
    want_s, want_l = sample(ref, b), eval_loss(ref, b)
    assert not torch.equal(want_s, live_s) and want_l != live_l
    with pol.ema_weights():
        in_s, in_l = sample(pol, b), eval_loss(pol, b)
        assert torch.equal(in_s, want_s) and in_l == want_l
        sel = pol.select_action(b["images"][0], b["states"][0], b["tasks"][0], torch.device(DEV))
        assert sel.shape == (14,) and bool(torch.isfinite(sel).all())
        with pytest.raises(RuntimeError, match="ema_weights"):
            pol.merge_lora()
    pol.reset()
    assert pol._ema_live().data_ptr() == live_ptr and torch.equal(pol._ema_live(), live_buf)
    assert torch.equal(sample(pol, b), live_s) and eval_loss(pol, b) == live_l
    # merge_lora on the flow policy: what it samples and what it loses stay
    pol.disable_ema() if hasattr(pol, "disable_ema") else None
    lb = [float(t.abs().max()) for k, t in pol._unfrozen.lora_state()["tensors"].items() if "lora_B" in k]
    assert len(lb) >= 7 and min(lb) > 0 and not pol._unfrozen.lora_adapters_zero          # three updates moved every lora_B off its zero start: there is something to merge
    pol.merge_lora()
    assert pol._unfrozen.lora_adapters_zero
    s2, l2 = sample(pol, b), eval_loss(pol, b)
    es, el = rel_l2(s2.cpu(), live_s.cpu()), abs(l2 - live_l) / live_l
    print(f"[flow merge_lora] sampled chunk (same offset) merged vs adapted: rel_l2 {es:.2e}; evaluation loss relative {el:.2e}")
    assert es <= 1e-5 and el <= 1e-5
    for p_ in (pol, ref):
        p_.model.backbone.engine().close()
