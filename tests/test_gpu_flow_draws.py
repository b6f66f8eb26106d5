"""-m gpu: several noise draws per observation in one flow-head training step (fv_head_set_flow_draws / flow_noise_draws).

Everything leans on one identity: draw s of an S-draw call at offset o is the single-draw call at offset o + (s << 56), head rows are draw-major (s B + b),
and an S-draw step is the mean of those S single-draw steps.  Bars are the existing ones, unchanged: x_t / u 0 ulp of the rounded float64 formula, phi
test_gpu_flow.SINCOS_ULP, the head step test_gpu_flow.test_flow_head_step_matches_float64_autograd's (loss 1e-5 relative, gradients 2e-5 of the largest
reference element), the routes test_gpu_flow.test_backbone_routes_noise_like_the_head_only_route's (velocity and loss 1e-3, gradients rel-L2 2e-3)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_draws_util as du  # noqa: E402
import flow_util as fu  # noqa: E402
from chunk_loss_util import ragged_pad  # noqa: E402
from gpu_util import DEV, lib, rel_l2, stream  # noqa: E402
from test_gpu_flow import SINCOS_ULP, _cat_view, _engine, _flat  # noqa: E402
from fastvla_hip import HEAD_KEYS, FastVLAEngine, _lib, arch  # noqa: E402
from fastvla_hip.engine import flow_draw_offset  # noqa: E402


def _draws_engine(name, B, S, **kw):
    eng = _engine(name, B, **kw)
    if S != 1:
        eng.set_head_flow_draws(S)
    return eng


def _cat_rows(eng, saved, B, S):
    """the (S B, cw) cat matrix inside `saved` (test_gpu_flow._cat_view finds its start with an inference forward, which fills rows 0 .. B - 1)"""
    off, _ = _cat_view(eng, saved, B)
    cw = eng.head_cat_width()
    return off, saved[off:off + S * B * cw].view(S * B, cw)


# ------------------------------------------------------------------------------------------------------------------ 1. prepare
@pytest.mark.parametrize("S", du.DRAWS)
@pytest.mark.parametrize("B", du.BATCHES)
@pytest.mark.parametrize("name", du.HEADS)
def test_prepare_with_explicit_noise_and_t(name, B, S):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da, R = K * A, S * B
    eng = _draws_engine(name, B, S)
    g = torch.Generator().manual_seed(5 + B + 7 * S)
    a, eps, t = torch.randn(B, da, generator=g), torch.randn(R, da, generator=g), torch.rand(R, generator=g)
    t[0] = 1.0
    t[R - 1] = 0.0
    if R > 2:
        eps[R - 2] = -a[(R - 2) % B] * 3                       # t eps and (1 - t) a cancel at t = 1 / 4, in the last draw
        t[R - 2] = 0.25
    saved = eng.head_saved(B)
    off, cat = _cat_rows(eng, saved, B, S)
    saved.fill_(float("nan"))
    u = eng.head_flow_prepare(a, saved, noise=eps, t=t)
    torch.cuda.synchronize()
    assert u.shape == (R, da) and cat.shape == (R, eng.head_cat_width())
    xo = feat + hid
    x_ref, u_ref = fu.noising_ref(np.tile(a.numpy(), (S, 1)), eps.numpy(), t.numpy())
    x_got, phi_got = cat[:, xo:xo + da].cpu().double().numpy(), cat[:, xo + da:].cpu().double().numpy()
    phi_ref = fu.phi_ref(t.numpy(), fu.flow_freqs(E))
    ep = np.abs(phi_got - phi_ref) / fu.ulp32(phi_ref)
    print(f"[flow draws prepare {name} B={B} S={S}] phi worst error {ep.max():.2f} ulp (bar {SINCOS_ULP})")
    assert np.array_equal(x_got, x_ref.astype(np.float32).astype(np.float64))          # 0 ulp: the float64 formula rounded once
    assert np.array_equal(u.cpu().double().numpy(), u_ref.astype(np.float32).astype(np.float64))
    assert ep.max() <= SINCOS_ULP
    # nothing but the two new column blocks of the S B cat rows was written (the conditioning columns of the later draws are the forward's to fill)
    mask = torch.ones_like(saved, dtype=torch.bool)
    mask.view(-1)[off:off + R * eng.head_cat_width()].view(R, -1)[:, xo:] = False
    assert bool(torch.isnan(saved[mask]).all()) and not bool(torch.isnan(saved[~mask]).any())
    # rows 0 .. B - 1 are the single-draw call's rows
    one = _draws_engine(name, B, 1)
    sv1 = one.head_saved(B)
    _, cat1 = _cat_rows(one, sv1, B, 1)
    u1 = one.head_flow_prepare(a, sv1, noise=eps[:B], t=t[:B])
    torch.cuda.synchronize()
    assert torch.equal(u1, u[:B]) and torch.equal(cat1[:, xo:], cat[:B, xo:])
    assert saved.numel() > sv1.numel() if S > 1 else saved.numel() == sv1.numel()
    eng.close(), one.close()


@pytest.mark.parametrize("S", du.DRAWS)
@pytest.mark.parametrize("name", du.HEADS)
def test_prepare_draws_follow_the_offset_rule(name, S):
    B, seed, o = 9, 0x1234_5678_9ABC, du.train_offset(5, 77, 2)
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da, xo = K * A, feat + hid
    eng, one = _draws_engine(name, B, S), _draws_engine(name, B, 1)

    def run(e, Bc, Sc, off_, noise=None):
        saved = e.head_saved(Bc)
        _, cat = _cat_rows(e, saved, Bc, Sc)
        u = e.head_flow_prepare(torch.zeros(Bc, da), saved, seed=seed, offset=off_, noise=noise)
        torch.cuda.synchronize()
        return cat[:, xo:].clone().cpu(), u.cpu()

    xt, _ = run(eng, B, S, o, noise=torch.ones(S * B, da))                          # a = 0, eps = 1: x_t = t exactly
    xn, un = run(eng, B, S, o)                                                       # a = 0: u = eps
    x3, u3 = run(eng, 3, S, o)
    worst = 0.0
    for s in range(S):
        rows = slice(s * B, (s + 1) * B)
        os_ = flow_draw_offset(o, s)
        assert os_ == o + (s << 56)
        assert np.array_equal(xt[rows, 0].numpy(), fu.draw_t_uniform(B, seed, os_))   # bit for bit
        n_ref, bar = fu.draw_normals(B, da, seed, os_)
        err = np.abs(un[rows].double().numpy() - n_ref)
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        assert bool((err <= bar).all())
        # draw s IS the single-draw call at o + (s << 56), and a row's draws do not depend on B
        x1, u1 = run(one, B, 1, os_)
        assert torch.equal(x1, xn[rows]) and torch.equal(u1, un[rows])
        assert torch.equal(x3[s * 3:(s + 1) * 3], xn[rows][:3]) and torch.equal(u3[s * 3:(s + 1) * 3], un[rows][:3])
    assert all(not torch.equal(un[:B], un[s * B:(s + 1) * B]) for s in range(1, S))
    print(f"[flow draws offsets {name} S={S}] worst normal error / bar {worst:.3f}")
    # bits 56 .. 59 belong to the draw index: refused with more than one draw (nothing enqueued), accepted with one
    saved = eng.head_saved(B).fill_(float("nan"))
    out = torch.full((S * B, da), float("nan"), device=DEV)
    tg = torch.zeros(B, da, device=DEV)
    rc = eng.lib.fv_head_flow_prepare(eng.h, tg.data_ptr(), B, seed, o | (1 << 57), None, None, saved.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    if S > 1:
        assert rc == -1 and b"56" in eng.lib.fv_last_error(eng.h) and bool(torch.isnan(saved).all()) and bool(torch.isnan(out).all())
    else:
        assert rc == 0 and not bool(torch.isnan(out).any())
    eng.close(), one.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the head step against float64 autograd
def _weights(A, K, seed):
    g = torch.Generator().manual_seed(seed)
    dim_w, step_w = torch.rand(A, generator=g) * 2.0 + 0.25, torch.rand(K, generator=g) * 2.0 + 0.25
    dim_w[A - 1] = 0.0                                          # a weight of 0 selects the element away
    return dim_w, step_w


def _op_backward(eng, dims, S, flat, v, u, pad, w, kind, B, saved):
    """fv_op_head_loss_backward_draws: the same launch_head_backward, handing out the folded (B, feat) d_pooled"""
    feat, ds, hid, fus, K, A, E = dims
    da, R = K * A, S * B
    G, dp = torch.zeros_like(flat), torch.full((B, feat), float("nan"), device=DEV)      # (zeros: the flat buffer has alignment gaps that nobody writes)
    loss, met = torch.zeros(1, device=DEV), torch.zeros(4, device=DEV)
    scr = torch.zeros(R * da + 2 * R * max(eng.head_cat_width(), fus) + 64 + 768 + (R * da + 3) // 4, device=DEV)
    padd = None if pad is None else torch.from_numpy(np.asarray(pad)).to(DEV, torch.uint8).contiguous()
    dw, sw = (None, None) if w is None else (w[0].to(DEV).contiguous(), w[1].to(DEV).contiguous())
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    _lib.check(lib().fv_op_head_loss_backward_draws(feat, ds, da, hid, fus, E, S, flat.data_ptr(), v.data_ptr(), u.data_ptr(), ptr(padd), ptr(dw), ptr(sw),
                                                    _lib.LOSS_KINDS[kind], 1.0, K, B, saved.data_ptr(), loss.data_ptr(), met.data_ptr(), G.data_ptr(), scr.data_ptr(),
                                                    scr.numel(), dp.data_ptr(), stream()), "fv_op_head_loss_backward_draws")
    torch.cuda.synchronize()
    return loss, G, dp


def _grad_bar(r):
    return 2e-5 * max(1e-3, float(r.abs().max()))


@pytest.mark.parametrize("kind,weighted", [("mse", False), ("mse", True), ("l1", True)])
@pytest.mark.parametrize("S", du.DRAWS)
@pytest.mark.parametrize("B", du.BATCHES)
@pytest.mark.parametrize("name", du.HEADS)
def test_head_step_matches_float64_autograd(name, B, S, kind, weighted):
    c = du.case(name, B, S)
    feat, ds, hid, fus, K, A, E = c["dims"]
    pad = ragged_pad(B, K, seed=1) if B * K > 1 else np.zeros((B, K), dtype=bool)
    w = _weights(A, K, 3) if weighted else None
    eng = _draws_engine(name, B, S)
    eng.set_head_loss(kind, 1.0, K)
    if w is not None:
        eng.set_head_loss_weights(*w)
    flat = _flat(eng, c["p"])
    saved = eng.head_saved(B)
    u = eng.head_flow_prepare(c["a"], saved, noise=c["eps"], t=c["t"])
    v, _ = eng.head_forward(flat, c["pooled"].to(DEV), c["states"].to(DEV), saved=saved, normalized_actions=True)
    loss, grads = eng.head_backward(flat, v, u, saved, pad=pad)
    torch.cuda.synchronize()
    assert v.shape == (S * B, K * A)
    ref = du.draws_reference(c["p"], c["pooled"], c["states"], c["a"], c["eps"], c["t"], pad, kind, S, c["dims"], *(w or (None, None)))
    np.testing.assert_allclose(v.cpu().numpy(), ref["pred"].numpy(), rtol=1e-4, atol=1e-5)
    el = abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    gv = eng.head_views(grads)
    worst = max(float((gv[k].cpu().double() - ref["grads"][k]).abs().max()) / _grad_bar(ref["grads"][k]) for k in HEAD_KEYS)
    loss2, G2, dp = _op_backward(eng, c["dims"], S, flat, v, u, pad, w, kind, B, saved)
    ed = float((dp.cpu().double() - ref["d_pooled"]).abs().max()) / _grad_bar(ref["d_pooled"])
    print(f"[flow draws head step {name} B={B} S={S} {kind} weighted={weighted}] loss rel {el:.2e}; worst gradient error / bar {worst:.3f}; d_pooled {ed:.3f}")
    assert el <= 1e-5
    for k in HEAD_KEYS:
        err = float((gv[k].cpu().double() - ref["grads"][k]).abs().max())
        assert err <= _grad_bar(ref["grads"][k]), (k, err, _grad_bar(ref["grads"][k]))
    assert all(torch.equal(t2, gv[k]) for k, t2 in eng.head_views(G2).items()) and torch.equal(loss2, loss)      # the test entry point runs the product's launch
    assert ed <= 1.0, ("d_pooled", ed)
    # the metrics and the per-dimension error run over all S B rows
    met = eng.head_loss_metrics().cpu().double()
    padt = torch.from_numpy(np.tile(pad, (S, 1)))
    d = (v.cpu().double() - u.cpu().double()).view(S * B, K, A)
    valid = (~padt).unsqueeze(-1).expand_as(d)
    assert abs(float(met[1]) - float((~padt).double().mean())) <= 1e-6          # the valid fraction counts every draw's rows
    if not weighted:
        mse = float((d * d)[valid].sum() / d.numel())
        assert abs(float(met[0]) - mse) <= 1e-5 * max(1e-3, mse)
    per = eng.head_loss_per_dim(v, u, pad=pad).cpu().double()
    want = torch.stack([d[..., j][~padt].abs().mean() if bool((~padt).any()) else torch.zeros((), dtype=torch.float64) for j in range(A)])
    assert float((per - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the mean-of-singles identity, head only
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("S", [2, 5, 8])
@pytest.mark.parametrize("B", du.BATCHES)
@pytest.mark.parametrize("name", du.HEADS)
def test_s_draw_step_is_the_mean_of_s_single_draw_steps(name, B, S, kind):
    """Internal draws, dropout 0.  The S-draw call at offset o against the mean of S single-draw calls at o + (s << 56), both against the float64 reference
    evaluated on the noise the device drew (read back exactly: targets 0 gives u = eps, noise 1 gives x_t = t).  The S-draw result is held to the head
    step's bar; every single-draw call is held to that bar against ITS reference, so their mean is within the mean of the S bars; the two GPU results are
    then within the sum of the two bars of each other.  All three are asserted."""
    c = du.case(name, B, S, seed=1)
    feat, ds, hid, fus, K, A, E = c["dims"]
    da, seed, o = K * A, 991, du.train_offset(3, 1000, 1)
    pad = ragged_pad(B, K, seed=2) if B * K > 1 else None
    eng, one = _draws_engine(name, B, S), _draws_engine(name, B, 1)
    for e in (eng, one):
        e.set_head_loss(kind, 1.0, K)
    flat = _flat(eng, c["p"])
    pooled, states = c["pooled"].to(DEV), c["states"].to(DEV)
    saved = eng.head_saved(B)
    xo = feat + hid
    _, cat = _cat_rows(eng, saved, B, S)
    eps = eng.head_flow_prepare(torch.zeros(B, da), saved, seed=seed, offset=o).cpu()
    eng.head_flow_prepare(torch.zeros(B, da), saved, seed=seed, offset=o, noise=torch.ones(S * B, da))
    torch.cuda.synchronize()
    t = cat[:, xo].clone().cpu()

    def step(e, off_):
        sv = e.head_saved(B)
        u = e.head_flow_prepare(c["a"], sv, seed=seed, offset=off_)
        v, _ = e.head_forward(flat, pooled, states, saved=sv, normalized_actions=True)
        loss, grads = e.head_backward(flat, v, u, sv, pad=pad)
        torch.cuda.synchronize()
        return float(loss), grads.clone(), v.clone()

    lm, gm, vm = step(eng, o)
    singles = [step(one, flow_draw_offset(o, s)) for s in range(S)]
    assert all(torch.equal(vm[s * B:(s + 1) * B], singles[s][2]) for s in range(S))      # every draw's prediction is the single-draw call's, bit for bit
    ls = sum(x[0] for x in singles) / S
    gs = sum(x[1].double() for x in singles) / S
    ref = du.mean_of_singles(c["p"], c["pooled"], c["states"], c["a"], eps, t, pad, kind, S, c["dims"])
    rl = float(ref["loss"])
    assert abs(lm - rl) <= 1e-5 * rl and abs(ls - rl) <= 1e-5 * rl and abs(lm - ls) <= 2e-5 * rl
    vm_, vs_ = eng.head_views(gm), eng.head_views(gs)
    worst = 0.0
    for k in HEAD_KEYS:
        r = ref["grads"][k]
        bar_m, bar_s = _grad_bar(r), sum(_grad_bar(x["grads"][k]) for x in ref["each"]) / S
        em, es = float((vm_[k].cpu().double() - r).abs().max()), float((vs_[k].cpu() - r).abs().max())
        eb = float((vm_[k].cpu().double() - vs_[k].cpu()).abs().max())
        worst = max(worst, em / bar_m, es / bar_s, eb / (bar_m + bar_s))
        assert em <= bar_m and es <= bar_s and eb <= bar_m + bar_s, (k, em, bar_m, es, bar_s, eb)
    print(f"[flow draws identity {name} B={B} S={S} {kind}] loss S-draw {lm:.6f} mean of singles {ls:.6f} float64 {rl:.6f}; worst error / bar {worst:.3f}")
    eng.close(), one.close()


# ------------------------------------------------------------------------------------------------------------------ 4. off means off
def test_off_means_off_and_the_setter_checks():
    name, B = "awkward", 5
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    c = du.case(name, B, 5)
    fresh, seen, never = _engine(name, B), _engine(name, B), _engine(name, B)
    L = seen.lib

    def sizes(e):
        n = C.c_size_t()
        assert L.fv_workspace_bytes(e.h, B, 8, 0, C.byref(n)) == 0
        return e.head_saved(B).numel(), n.value

    # every bad call: its code, nothing changed
    for bad in (0, 17, -1, 1 << 20):
        assert L.fv_head_set_flow_draws(seen.h, bad) == -1 and b"fv_head_set_flow_draws" in L.fv_last_error(seen.h), bad
    assert L.fv_head_set_flow_draws(None, 2) == -1
    reg = _engine(name, B, flow=False)
    assert L.fv_head_set_flow_draws(reg.h, 2) == -2 and L.fv_head_set_flow_draws(reg.h, 1) == -2      # the regression head has no noise
    assert sizes(seen) == sizes(fresh)
    with pytest.raises(ValueError):
        seen.set_head_flow_draws(0)
    # 3, then 1: the bytes, the loss and the gradients of a fresh handle; a handle that never made the call matches too
    seen.set_head_flow_draws(3)
    assert seen.head_flow_draws == 3 and sizes(seen)[0] > sizes(fresh)[0] and sizes(seen)[1] >= sizes(fresh)[1]
    seen.set_head_flow_draws(1)
    assert sizes(seen) == sizes(fresh) == sizes(never)
    never.set_head_flow(None)                                   # fv_head_set_flow(NULL) resets the draws as well
    never.set_head_flow(E)
    assert never.head_flow_draws == 1 and sizes(never) == sizes(fresh)
    outs = []
    for e in (fresh, seen, never):
        e.set_head_loss("l1", 1.0, K)
        flat = _flat(e, c["p"])
        sv = e.head_saved(B)
        u = e.head_flow_prepare(c["a"], sv, seed=3, offset=9)
        v, _ = e.head_forward(flat, c["pooled"].to(DEV), c["states"].to(DEV), training=True, dropout_p=0.1, seed=7, offset=3, saved=sv)
        loss, grads = e.head_backward(flat, v, u, sv, dropout_p=0.1, pad=ragged_pad(B, K, seed=1))
        torch.cuda.synchronize()
        outs.append((u.clone(), v.clone(), loss.clone(), grads.clone()))
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1])) and all(torch.equal(x, y) for x, y in zip(outs[0], outs[2]))
    # the workspace is bound now: sizes depend on the setting, so the setter refuses
    assert L.fv_head_set_flow_draws(seen.h, 2) == -2 and b"fv_bind_workspace" in L.fv_last_error(seen.h)
    assert L.fv_head_set_flow_draws(seen.h, 1) == -2
    # two S = 5 calls give the same bits; the sampler ignores the setting
    five = _draws_engine(name, B, 5)
    five.set_head_loss("l1", 1.0, K)
    flat = _flat(five, c["p"])
    runs = []
    for _ in range(2):
        sv = five.head_saved(B)
        u = five.head_flow_prepare(c["a"], sv, seed=3, offset=9)
        v, _ = five.head_forward(flat, c["pooled"].to(DEV), c["states"].to(DEV), training=True, dropout_p=0.1, seed=7, offset=3, saved=sv)
        loss, grads = five.head_backward(flat, v, u, sv, dropout_p=0.1, pad=ragged_pad(B, K, seed=1))
        torch.cuda.synchronize()
        runs.append((u.clone(), v.clone(), loss.clone(), grads.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs)) and runs[0][1].shape == (5 * B, da)
    assert torch.equal(runs[0][0][:B], outs[0][0]) and torch.equal(runs[0][1][:B], outs[0][1])      # rows 0 .. B - 1: the single-draw call's, dropout mask included
    sc = fu.sampler_case(name, B)
    fl1, fl5 = _flat(fresh, sc["p"]), _flat(five, sc["p"])
    for kw in (dict(noise=sc["noise"]), dict(seed=3, offset=4)):
        s1 = fresh.head_flow_sample(fl1, sc["pooled"].to(DEV), sc["states"].to(DEV), steps=4, **kw)
        s5 = five.head_flow_sample(fl5, sc["pooled"].to(DEV), sc["states"].to(DEV), steps=4, **kw)
        torch.cuda.synchronize()
        assert s5.shape == (B, da) and torch.equal(s1, s5)
    for e in (fresh, seen, never, reg, five):
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 5. isolation
@pytest.mark.parametrize("S", du.DRAWS)
def test_rows_and_draws_stay_isolated(S):
    """(a) The mask is (B, K) and applies to every draw of its observation: NaN in the LOSS targets (u) at the padded steps of one observation, in every
    draw's row, changes no bit of the loss, the metrics, the 12 gradients or d_pooled.  (NaN in the padded steps of the raw action targets is another
    matter at any S, 1 included: x_t = t eps + (1 - t) a is the network's input, so it reaches that observation's prediction by the definition of noising.)
    (b) NaN in one observation's VALID target reaches that observation's d_pooled row only: the other rows keep their bits."""
    name, B, kind = "awkward", 9, "l1"
    c = du.case(name, B, S, seed=2)
    feat, ds, hid, fus, K, A, E = c["dims"]
    pad = ragged_pad(B, K, seed=1)
    j = int(np.flatnonzero(pad.any(1) & ~pad.all(1))[0])        # an observation with both valid and padded steps
    eng = _draws_engine(name, B, S)
    eng.set_head_loss(kind, 1.0, K)
    flat = _flat(eng, c["p"])

    def run(a, poison_u):
        saved = eng.head_saved(B)
        u = eng.head_flow_prepare(a, saved, noise=c["eps"], t=c["t"])
        v, _ = eng.head_forward(flat, c["pooled"].to(DEV), c["states"].to(DEV), saved=saved, normalized_actions=True)
        if poison_u:
            uv = u.view(S, B, K, A)
            uv[:, j][:, torch.from_numpy(pad[j]).to(DEV)] = float("nan")
        loss, grads = eng.head_backward(flat, v, u, saved, pad=pad)
        met = eng.head_loss_metrics().clone()
        loss2, G2, dp = _op_backward(eng, c["dims"], S, flat, v, u, pad, None, kind, B, saved)
        return loss.clone(), met, grads.clone(), dp.clone(), loss2.clone(), G2.clone()

    clean, poisoned = run(c["a"], False), run(c["a"], True)
    assert all(torch.equal(x, y) for x, y in zip(clean, poisoned)) and bool(torch.isfinite(clean[2]).all()) and bool(torch.isfinite(clean[3]).all())
    a_bad = c["a"].clone()
    a_bad.view(B, K, A)[j, 0, 0] = float("nan")                  # step 0 of observation j is valid
    assert not pad[j, 0]
    bad = run(a_bad, False)
    others = [b for b in range(B) if b != j]
    assert bool(torch.isnan(bad[3][j]).all()) and torch.equal(bad[3][others], clean[3][others])
    assert bool(torch.isnan(bad[0]).all())                       # (the loss and the 12 gradients are sums over all rows)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. the backbone routes
def _route_rig(model, seed, hd, B, T, da, E, S):
    from test_gpu_flow import _route_rig as rig
    from fastvla_hip import weights
    if S == 1:
        return rig(model, seed, hd, B, T, da, E)
    # test_gpu_flow._route_rig with the draws set where they have to be: before train_begin
    w = weights.init_backbone(model, seed=seed)
    eng = FastVLAEngine(model, state_dim=14, action_dim=da, hidden_dim=hd, fusion_dim=hd, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng.set_head_flow(E)
    eng.set_head_flow_draws(S)
    eng.load_weights(w)
    eng.train_begin()
    _, total, _ = eng.train_layout()
    flat = torch.zeros(total, dtype=torch.float32, device=DEV)
    eng.train_export_params(flat)
    g = torch.Generator().manual_seed(seed + 1)
    shapes = fu.flow_head_shapes(model.llm.hidden, 14, da, hd, hd, E)
    hp = {k: (torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
          for k, s in shapes.items()}
    for k, v in eng.head_views(flat).items():
        v.copy_(hp[k])
    return w, eng, flat


ROUTE = dict(B=3, T=16, K=4, A=5, hd=64, E=6, rank=16, seed=1234, offset=du.train_offset(2, 40, 1))


def _route_steps(S, offsets):
    """one rig with S draws: a full fine-tuning step, a rank-16 projected LoRA step and a direct LoRA step per offset, the same weights throughout (no optimiser
    step in between) -> per offset {"full" | "proj" | "direct": (velocity, loss, gradients / loss scale)}, plus the head-only route's results on the same draws"""
    from oracle import fastvit_hd
    from test_gpu_lora import _random_adapters
    from test_gpu_train_unfrozen import _inputs
    r = ROUTE
    model = arch.preset("small")
    B, T, K, da = r["B"], r["T"], r["K"], r["K"] * r["A"]
    w, eng, flat = _route_rig(model, 41, r["hd"], B, T, da, r["E"], S)
    tower_out, ids, mask, states, _ = _inputs(model, B, T, 42)
    targets = torch.randn(B, da, generator=torch.Generator().manual_seed(43))
    eng.set_head_loss("mse", 1.0, K)
    ws = eng.train_workspace(B, T)
    scale = eng.train_loss_scale()
    common = (tower_out.to(DEV), ids, mask.sum(1), states, targets, ws)

    def head_only(off_):
        with torch.no_grad():
            tok = fastvit_hd.projector_forward(w, tower_out.float()).to(DEV)
        pooled = eng.llm_pooled(ids, mask.sum(1), tok)
        hflat = flat[: eng.head_numel()].clone()
        saved = eng.head_saved(B)
        u = eng.head_flow_prepare(targets, saved, seed=r["seed"], offset=off_)
        v, _ = eng.head_forward(hflat, pooled, states.to(DEV), saved=saved, normalized_actions=True)
        loss, grads = eng.head_backward(hflat, v, u, saved)
        torch.cuda.synchronize()
        return v[:B].clone(), float(loss), grads.clone()

    out = {o: {} for o in offsets}
    for o in offsets:
        out[o]["head_full"] = head_only(o)
        a, l, g = eng.train_forward_backward(flat, *common, training=False, seed=r["seed"], offset=o, flat_grads=torch.zeros_like(flat))
        torch.cuda.synchronize()
        out[o]["full"] = (a.clone(), float(l), g / scale)
    eng.train_lora_begin(r["rank"], 2.0 * r["rank"], None)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    _random_adapters(eng, lflat, lt, seed=9)
    eng.train_lora_commit(flat, lflat)
    for o in offsets:
        out[o]["head_lora"] = head_only(o)                       # (the inference forward now runs the adapted weights)
        a, l, g = eng.train_forward_backward(flat, *common, training=False, seed=r["seed"], offset=o, flat_grads=torch.zeros_like(flat))
        lg = torch.zeros_like(lflat)
        eng.train_lora_project(g, lflat, lg)
        torch.cuda.synchronize()
        out[o]["proj"] = (a.clone(), float(l), lg / scale)
        a, l, g = eng.train_lora_forward_backward(flat, lflat, *common, training=False, seed=r["seed"], offset=o, lora_grads=torch.zeros_like(lflat))
        torch.cuda.synchronize()
        out[o]["direct"] = (a.clone(), float(l), g / scale)
    layouts = {"full": eng.train_layout()[0], "proj": lt, "direct": lt}
    views = lambda g: {k: t.clone() for k, t in eng.head_views(g[: eng.head_numel()]).items()}  # noqa: E731
    hn = eng.head_numel()
    # an offset that uses the draw bits is refused before anything is enqueued, on both entry points: the gradient buffers keep their NaN
    if S > 1:
        gb, lb = torch.full_like(flat, float("nan")), torch.full_like(lflat, float("nan"))
        with pytest.raises(_lib.FastVLAHipError, match="56"):
            eng.train_forward_backward(flat, *common, training=False, seed=r["seed"], offset=offsets[0] | (1 << 57), flat_grads=gb)
        with pytest.raises(_lib.FastVLAHipError, match="56"):
            eng.train_lora_forward_backward(flat, lflat, *common, training=False, seed=r["seed"], offset=offsets[0] | (1 << 57), lora_grads=lb)
        torch.cuda.synchronize()
        assert bool(torch.isnan(gb).all()) and bool(torch.isnan(lb).all())
    eng.close()
    return out, layouts, views, hn


@pytest.fixture(scope="module")
def single_draw_routes():
    """the five single-draw steps at o + (s << 56) on every route: computed once, shared by S = 2 and S = 5, never modified"""
    offs = [flow_draw_offset(ROUTE["offset"], s) for s in range(5)]
    out, layouts, views, hn = _route_steps(1, offs)
    return [out[o] for o in offs]


@pytest.mark.parametrize("S", [2, 5])
def test_backbone_routes_take_s_draws_for_one_backbone_pass(S, single_draw_routes):
    from test_gpu_train_unfrozen import GRAD_TOL
    o = ROUTE["offset"]
    out, layouts, views, hn = _route_steps(S, [o])
    multi, singles = out[o], single_draw_routes[:S]
    for route in ("full", "proj", "direct"):
        v, loss, g = multi[route]
        v0 = singles[0][route][0]
        lmean = sum(x[route][1] for x in singles) / S
        gmean = sum(x[route][2].double() for x in singles) / S
        ev, el = rel_l2(v.cpu(), v0.cpu()), abs(loss - lmean) / lmean
        errs = []
        for t in layouts[route]:
            a, b = g[t["offset"]:t["offset"] + t["numel"]].double(), gmean[t["offset"]:t["offset"] + t["numel"]]
            if float(b.norm()) > 0:
                errs.append((rel_l2(a.cpu(), b.cpu()), t["name"]))
        errs.sort(reverse=True)
        print(f"[flow draws route {route} S={S}] velocity (draw 0) rel_l2 {ev:.2e} loss rel {el:.2e} ({loss:.6f} vs mean of singles {lmean:.6f}); "
              f"{len(errs)} gradient tensors, worst: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
        assert v.shape == (ROUTE["B"], ROUTE["K"] * ROUTE["A"]) and ev <= 1e-3 and el <= 1e-3
        assert len(errs) >= 12
        for e, k in errs:
            assert e <= GRAD_TOL, (route, k, e)
    # the head section against the head-only route on the same draws and an inference forward's pooled feature
    for route, ref in (("full", "head_full"), ("proj", "head_lora")):
        v, loss, g = multi[route]
        rv, rl, rg = multi[ref]
        got, want = views(g), views(rg)
        errs = sorted(((rel_l2(got[k].cpu(), want[k].cpu()), k) for k in HEAD_KEYS), reverse=True)
        ra, el = rel_l2(v.cpu(), rv.cpu()), abs(loss - rl) / rl
        print(f"[flow draws route {route} S={S} vs head-only] velocity rel_l2 {ra:.2e} loss rel {el:.2e}; worst head gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
        assert ra <= 1e-3 and el <= 1e-3 and all(e <= GRAD_TOL for e, _ in errs), errs[:3]
    # the direct step's head gradients, loss and velocity are the projected step's, bit for bit
    assert torch.equal(multi["direct"][0], multi["proj"][0]) and multi["direct"][1] == multi["proj"][1]
    assert torch.equal(multi["direct"][2][:hn], multi["proj"][2][:hn])


# ------------------------------------------------------------------------------------------------------------------ 7. the policy level
def _policy(K=3, seed=31, draws=4, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K, n_action_steps=1,
                         action_head="flow", flow_time_dim=6, flow_seed=77, flow_noise_draws=draws, **kw).to(DEV)


def test_policy_trains_resumes_and_evaluates_with_four_draws(tmp_path, monkeypatch):
    """synthetic:tiny, head-only, K = 3, S = 4: three updates, save, resume in a fresh policy (S passed again: a property of the run), two more == an
    uninterrupted five-update run bit for bit in p, m, v; eval() compute_loss repeats its loss; the velocity handed out stays (B, K, A)."""
    from test_gpu_flow import _batch, _dev
    from vla_fastvlm.training import Trainer, TrainingConfig
    for k in ("FASTVLA_ACTION_HEAD", "FASTVLA_EMA_DECAY", "FASTVLA_FLOW_NOISE_DRAWS"):
        monkeypatch.delenv(k, raising=False)
    K, B, S = 3, 4, 4
    data = [_batch(B, K, s) for s in (31, 32, 33, 34, 35)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1, eval_steps=1000, seed=1)
    a = _policy(K)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=5, **tkw)).fit()
    b = _policy(K)
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=5, **tkw))
    tb.num_training_steps = 5
    tb.fit()
    c = _policy(K, seed=99)
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=5, resume_from=str(tmp_path / "b" / "checkpoints" / "step-3"), **tkw))
    tc.num_training_steps = 5
    tc.fit()
    torch.cuda.synchronize()
    assert c._opt_state["step"] == 5 and a.model._engine().head_flow_draws == S and c.model._engine().head_flow_draws == S
    assert torch.equal(c.model._flat, a.model._flat) and torch.equal(c._opt_state["m"], a._opt_state["m"]) and torch.equal(c._opt_state["v"], a._opt_state["v"])
    # the draws matter: the same five updates with one draw end elsewhere
    d = _policy(K, draws=1)
    Trainer(d, data, None, TrainingConfig(output_dir=str(tmp_path / "d"), save_steps=1000, max_steps=5, **tkw)).fit()
    assert not torch.equal(d.model._flat, a.model._flat)
    # one more step by hand: shapes, and the loss is the S-draw loss of the engine's own route
    batch = _dev(_batch(B, K, 5))
    a.train()
    out = a.fused_train_step(batch, lr=1e-3)
    torch.cuda.synchronize()
    assert out["actions"].shape == (B, K, 14) and float(out["loss"]) > 0
    res = a.compute_loss(batch)                                 # train() mode, outside the native step: differentiable w.r.t. the head
    res["loss"].backward()
    assert all(p_.grad is not None and float(p_.grad.abs().max()) > 0 for p_ in a.model.head_parameters())
    a.eval()
    with torch.no_grad():
        e1 = [float(a.compute_loss(bb)["loss"]) for bb in (batch, batch)]
    a.eval()
    with torch.no_grad():
        e2 = [float(a.compute_loss(bb)["loss"]) for bb in (batch, batch)]
        images, states = a.processor.prepare_images(batch["images"], DEV), a.processor.prepare_states(batch["states"], DEV)
        tasks = a.processor.prepare_tasks(batch["tasks"], batch_size=B)
        _, vel = a.model.forward_loss(images, states, tasks, batch["actions"], device=DEV, pad=batch["action_is_pad"])
    assert e1 == e2 and e1[0] != e1[1] and vel.shape == (B, K, 14)
    for p_ in (a, b, c, d):
        p_.model.backbone.engine().close()
